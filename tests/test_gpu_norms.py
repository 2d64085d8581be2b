"""matrix_norm / matrix_norm_device / pxlange / pxlanhe / pxlantr on the GPU (one process) against numpy on the FULL
matrix -- built from the stored triangle for the Hermitian ('H') and the triangular ('T') structure.

Exact operands (small integers times powers of two; complex entries purely real or purely imaginary): every sum is
exact in fp64 and in the float result, so M, 1 and I must equal the reference (math.fsum) bit for bit and F within 2 ulp
of the result type.  Uniform operands: bounds derived from the any-order error bound of a sum of non-negative terms,
u = 2^-53, v = 2^-24 for s / c (the final rounding to float) and 0 for d / z:
    M   real: equality;  complex: relative error <= 4 2^-52 + v       (the accuracy the device hypot documents)
    1,I relative error <= (N + 8) u + v  (+ 4 2^-52 for complex: one modulus per term), N = terms of the winning sum
    F   relative error <= (N_sq / 2 + 8) u + v, N_sq = real squares summed (stored elements; re and im count apart)
against a longdouble reference.  Nothing outside the referenced part (other triangle, unit diagonal, imaginary part of a
Hermitian diagonal, rows beyond m) may change a value, and the caller's array and a resident matrix stay bit-identical.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
NORMS = ["M", "1", "I", "F"]
# (structure, uplo, diag)
COMBOS = [("G", "L", "N"), ("H", "L", "N"), ("H", "U", "N"), ("T", "L", "N"), ("T", "L", "U"), ("T", "U", "N"),
          ("T", "U", "U")]
SQUARE = [(64, 64, 64), (333, 333, 100), (130, 130, 50), (1100, 1100, 256)]
GENERAL = SQUARE + [(130, 67, 64), (67, 130, 64), (1, 300, 64), (300, 1, 64), (1100, 900, 256)]
U53 = 2.0 ** -53


def shapes_of(structure):
    return GENERAL if structure == "G" else SQUARE


EXACT_CASES = [(t, c, sh) for t in "sdcz" for c in COMBOS for sh in shapes_of(c[0])]


def fortran(a):
    """a column-major copy with unit row stride whatever the shape (numpy keeps C strides for a one-row array)"""
    out = np.empty(a.shape, dtype=a.dtype, order="F")
    out[...] = a
    return out


def same_bits(x, y):
    return x.shape == y.shape and x.tobytes(order="F") == y.tobytes(order="F")


def cid(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


# ---------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def exact_operand(t, m, n, hermitian):
    """small integers times powers of two, two heavy rows (so that the one and the infinity norm of a triangle differ);
    complex entries purely real or purely imaginary; a Hermitian operand's diagonal carries an imaginary part that must
    be ignored"""
    rng = np.random.default_rng(1000 * m + n + ord(t))
    k = rng.integers(-8, 9, (m, n)).astype(np.float64) * 2.0 ** rng.integers(-2, 3, (m, n))
    for r in {min(1, m - 1), max(m - 2, 0)}:
        k[r, :] = 32.0 * rng.choice([-1.0, 1.0], n)
    if t in "cz":
        a = np.where(rng.integers(0, 2, (m, n)) == 1, k + 0j, 1j * k)
        if hermitian:
            a[np.diag_indices(min(m, n))] = np.diag(k) + 3j
    else:
        a = k
    a = fortran(a.astype(DT[t]))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def uniform_operand(t, m, n, scale_exp=0):
    rng = np.random.default_rng(77 + 1000 * m + n + ord(t))
    a = rng.uniform(-1, 1, (m, n))
    if t in "cz":
        a = a + 1j * rng.uniform(-1, 1, (m, n))
    a = fortran((a.astype(DT[t]) * DT[t](2.0 ** scale_exp)).astype(DT[t]))
    a.setflags(write=False)
    return a


def referenced(a, structure, uplo, diag, wide):
    """(full matrix the norm is of in `wide` precision, number of stored elements the device reads for it with the
    diagonal of a Hermitian matrix counted as real)"""
    cx = np.iscomplexobj(a)
    w = a.astype(wide)
    m, n = a.shape
    if structure == "G":
        return w, (2 if cx else 1) * m * n
    tri = np.tril(w) if uplo == "L" else np.triu(w)
    d = np.diag(w).copy()
    off = tri - np.diag(d)
    nsq_off = (2 if cx else 1) * (n * (n - 1) // 2)
    if structure == "H":
        return off + off.conj().T + np.diag(d.real.astype(wide)), nsq_off + n
    if diag == "U":
        return off + np.eye(n, dtype=wide), nsq_off + (2 if cx else 1) * n
    return tri, nsq_off + (2 if cx else 1) * n


def counted(structure, uplo, m, n):
    """mask of the elements of the full matrix that are terms of a column / row sum"""
    if structure == "T":
        return np.tril(np.ones((n, n), bool)) if uplo == "L" else np.triu(np.ones((n, n), bool))
    return np.ones((m, n), bool)


def exact_reference(a, structure, uplo, diag):
    """{norm: value} with exact sums (math.fsum of float64 terms that are exact themselves)"""
    full, _ = referenced(a, structure, uplo, diag, np.complex128 if np.iscomplexobj(a) else np.float64)
    absm = np.abs(full.real) + np.abs(full.imag) if np.iscomplexobj(full) else np.abs(full)  # one part is zero: exact
    sq = full.real ** 2 + full.imag ** 2 if np.iscomplexobj(full) else full ** 2
    ref = {"M": float(absm.max()),
           "1": max(math.fsum(c) for c in absm.T),
           "I": max(math.fsum(r) for r in absm),
           "F": math.sqrt(math.fsum(sq.ravel()))}
    return ref


@functools.lru_cache(maxsize=None)
def exact_reference_of(t, combo, shape):
    m, n, _ = shape
    return exact_reference(exact_operand(t, m, n, combo[0] == "H"), *combo)


def wide_reference(a, structure, uplo, diag):
    """{norm: (longdouble value, N of the bound)}"""
    cx = np.iscomplexobj(a)
    full, nsq = referenced(a, structure, uplo, diag, np.clongdouble if cx else np.longdouble)
    absm = np.abs(full)
    mask = counted(structure, uplo, *a.shape)
    cs, rs = absm.sum(axis=0), absm.sum(axis=1)
    sq = (full.real ** 2 + full.imag ** 2) if cx else full ** 2
    return {"M": (absm.max(), 0),
            "1": (cs.max(), int(mask[:, int(cs.argmax())].sum())),
            "I": (rs.max(), int(mask[int(rs.argmax()), :].sum())),
            "F": (np.sqrt(sq.sum()), nsq)}


def bound(t, norm, count):
    v = 2.0 ** -24 if t in "sc" else 0.0
    hyp = 4 * 2.0 ** -52 if t in "cz" else 0.0
    if norm == "M":
        return hyp + v if t in "cz" else 0.0
    if norm == "F":
        return (count / 2 + 8) * U53 + v
    return (count + 8) * U53 + v + hyp


def rel_err(value, ref):
    return float(abs(np.longdouble(value) - ref) / ref)


def result_type(t):
    return np.float32 if t in "sc" else np.float64


def norm_of(dlaf, grid, norm, a, nb, combo):
    return dlaf.matrix_norm(grid, norm, a, nb, structure=combo[0], uplo=combo[1], diag=combo[2])


def assert_exact(t, norm, value, ref, what):
    rt = result_type(t)
    want = float(rt(ref))
    print(f"{what} {norm}: device {value!r} reference {want!r}")
    if norm == "F":
        assert abs(value - want) <= 2 * float(np.spacing(rt(want))), (what, norm, value, want)
    else:
        assert value == want, (what, norm, value, want)


# ---------------------------------------------------------------------------------------------------- (1) exact operands
@pytest.mark.parametrize("t,combo,shape", EXACT_CASES, ids=cid)
def test_exact_operands(dlaf, grid, t, combo, shape):
    m, n, nb = shape
    a = exact_operand(t, m, n, combo[0] == "H")
    ref = exact_reference_of(t, combo, shape)
    if combo[0] == "T" and n > 1:
        assert ref["1"] != ref["I"], "the operand cannot tell the one norm from the infinity norm"
    for norm in NORMS:
        assert_exact(t, norm, norm_of(dlaf, grid, norm, a, nb, combo), ref[norm], (t, combo, shape))


# ---------------------------------------------------------------------------------------------------- (2) unreferenced memory
@pytest.mark.parametrize("t,combo,shape", [(t, c, sh) for t in "sdcz" for c in COMBOS
                                           for sh in ([(333, 333, 100), (130, 67, 64)] if c[0] == "G" else [(333, 333, 100)])],
                         ids=cid)
def test_unreferenced_memory_is_not_read(dlaf, grid, t, combo, shape):
    m, n, nb = shape
    structure, uplo, diag = combo
    src = exact_operand(t, m, n, structure == "H")
    nan = DT[t](np.nan + 1j * np.nan) if t in "cz" else DT[t](np.nan)
    big = np.full((m + 5, n), nan, dtype=DT[t], order="F")  # rows beyond m: ld > m
    a = big[:m, :]
    a[...] = src
    if structure != "G":
        other = np.triu(np.ones((n, n), bool), 1) if uplo == "L" else np.tril(np.ones((n, n), bool), -1)
        a[other] = nan
        idx = np.diag_indices(n)
        if structure == "T" and diag == "U":
            a[idx] = nan
        if structure == "H" and t in "cz":
            a.imag[idx] = np.nan
    before = big.copy(order="F")
    ref = exact_reference_of(t, combo, shape)
    for norm in NORMS:
        assert_exact(t, norm, norm_of(dlaf, grid, norm, a, nb, combo), ref[norm], (t, combo, shape))
    assert same_bits(big, before), "the caller's array was written"


# ---------------------------------------------------------------------------------------------------- (3) NaN and Inf
SPECIAL = [("G", "L", "N", (130, 67, 64), "last"), ("H", "L", "N", (333, 333, 100), "last"),
           ("T", "L", "N", (333, 333, 100), "last"), ("H", "L", "N", (333, 333, 100), "lower"),
           ("H", "U", "N", (333, 333, 100), "lower"), ("T", "U", "N", (333, 333, 100), "last")]


@pytest.mark.parametrize("t", "sdcz")
@pytest.mark.parametrize("case", SPECIAL, ids=cid)
def test_nan_and_inf(dlaf, grid, t, case):
    structure, uplo, diag, (m, n, nb), where = case
    combo = (structure, uplo, diag)
    a = np.array(exact_operand(t, m, n, structure == "H"), order="F")
    # the last element of the last ragged tile, or an element of a strictly-lower off-diagonal tile of the stored triangle
    i, j = (m - 1, n - 1) if where == "last" else ((250, 30) if uplo == "L" else (30, 250))
    for special, check in ((-np.inf, lambda v: v == np.inf), (np.nan, math.isnan)):
        a[i, j] = special
        for norm in NORMS:
            v = norm_of(dlaf, grid, norm, a, nb, combo)
            print(case, t, special, norm, v)
            assert check(v), (case, t, special, norm, v)
    if t in "cz":  # a NaN imaginary part beside an infinite real part is still a NaN -- unless a Hermitian diagonal holds it
        a[i, j] = complex(np.inf, np.nan)
        want_nan = not (structure == "H" and i == j)
        for norm in NORMS:
            v = norm_of(dlaf, grid, norm, a, nb, combo)
            assert math.isnan(v) if want_nan else v == np.inf, (case, t, norm, v)


# ---------------------------------------------------------------------------------------------------- (4) range
@pytest.mark.parametrize("t,exp", [("d", 500), ("d", -500), ("z", 500), ("z", -500), ("s", 60), ("s", -60), ("c", 60),
                                   ("c", -60)])
@pytest.mark.parametrize("combo", [COMBOS[0], COMBOS[1], COMBOS[5]], ids=cid)
def test_frobenius_range(dlaf, grid, t, exp, combo):
    m, n, nb = 333, 333, 100
    a = uniform_operand(t, m, n, exp)
    ref, nsq = wide_reference(a, *combo)["F"]
    v = norm_of(dlaf, grid, "F", a, nb, combo)
    err = rel_err(v, ref)
    print(f"F range {t} 2^{exp} {combo}: device {v!r} reference {float(ref)!r} rel err {err:.3e} bound {bound(t, 'F', nsq):.3e}")
    assert math.isfinite(v) and v > 0
    assert err <= bound(t, "F", nsq)


# ---------------------------------------------------------------------------------------------------- (5), (6) bounds, determinism
@pytest.mark.parametrize("t", "sdcz")
@pytest.mark.parametrize("combo", COMBOS, ids=cid)
def test_uniform_operands_within_derived_bounds_and_deterministic(dlaf, grid, t, combo):
    m, n, nb = (1100, 900, 256) if combo[0] == "G" else (1100, 1100, 256)
    a = uniform_operand(t, m, n)
    ref = wide_reference(a, *combo)
    for norm in NORMS:
        v = norm_of(dlaf, grid, norm, a, nb, combo)
        again = norm_of(dlaf, grid, norm, a, nb, combo)
        want, count = ref[norm]
        err, b = rel_err(v, want), bound(t, norm, count)
        print(f"{t} {combo} {norm}: device {v!r} reference {float(want)!r} rel err {err:.3e} bound {b:.3e} (N {count})")
        assert np.float64(v).tobytes() == np.float64(again).tobytes(), (norm, v, again)
        if b == 0.0:
            assert v == float(want), (norm, v, want)
        else:
            assert err <= b, (norm, v, want, err, b)


# ---------------------------------------------------------------------------------------------------- (7) resident operands
@pytest.mark.parametrize("t", "dz")
@pytest.mark.parametrize("uplo", "LU")
def test_resident_hermitian_matrix_and_its_factor(dlaf, grid, t, uplo):
    n, nb = 600, 256
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (n, n)) + (1j * rng.uniform(-1, 1, (n, n)) if t == "z" else 0)
    h = np.asfortranarray(((x + x.conj().T) / 2 + n * np.eye(n)).astype(DT[t]))
    A = dlaf.DeviceMatrix(grid, DT[t], uplo, n, nb)
    A.upload(h)

    def check(structure, diag):
        before = np.zeros((n, n), DT[t], order="F")
        A.download(before)
        ref = wide_reference(before, structure, uplo, diag)
        for norm in NORMS:
            v = dlaf.matrix_norm_device(norm, A, structure, diag)
            want, count = ref[norm]
            err, b = rel_err(v, want), bound(t, norm, count)
            print(f"resident {t} {uplo} {structure} {diag} {norm}: device {v!r} reference {float(want)!r} rel err {err:.3e}")
            assert (v == float(want)) if b == 0.0 else (err <= b), (structure, norm, v, want, err, b)
        after = np.zeros((n, n), DT[t], order="F")
        A.download(after)
        assert same_bits(before, after), "the resident matrix changed"

    check("H", "N")
    assert A.factorize() == 0
    check("T", "N")
    check("T", "U")
    A.close()


@pytest.mark.parametrize("t", "sdcz")
def test_resident_general_matrix(dlaf, grid, t):
    m, n, nb = 700, 300, 128
    a = uniform_operand(t, m, n)
    B = dlaf.GeneralDeviceMatrix(grid, DT[t], m, n, nb)
    B.upload(np.array(a, order="F"))
    ref = wide_reference(a, "G", "L", "N")
    for norm in NORMS:
        v = dlaf.matrix_norm_device(norm, B)
        want, count = ref[norm]
        err, b = rel_err(v, want), bound(t, norm, count)
        print(f"resident general {t} {norm}: device {v!r} reference {float(want)!r} rel err {err:.3e} bound {b:.3e}")
        assert (v == float(want)) if b == 0.0 else (err <= b), (norm, v, want, err, b)
        assert v == dlaf.matrix_norm(grid, norm, a, nb), "host and resident operands disagree"
    back = np.zeros((m, n), DT[t], order="F")
    B.download(back)
    assert same_bits(back, a), "the resident matrix changed"
    B.close()


# ---------------------------------------------------------------------------------------------------- (8) ScaLAPACK entries
@pytest.mark.parametrize("t", "sdcz")
def test_scalapack_entries_and_letters(dlaf, grid, t):
    n, nb = 130, 64
    a = exact_operand(t, n, n, False)
    h = exact_operand(t, n, n, True)
    desc = [1, grid.context, n, n, nb, nb, 0, 0, n]
    letters = {"M": "Mm", "1": "1Oo", "I": "Ii", "F": "FfEe"}
    for norm, alts in letters.items():
        g = dlaf.matrix_norm(grid, norm, a, nb)
        for letter in alts:
            assert dlaf.pxlange(letter, n, n, a, 1, 1, desc) == g, (norm, letter)
            assert dlaf.matrix_norm(grid, letter, a, nb) == g, (norm, letter)
        for uplo in "LU":
            want = dlaf.matrix_norm(grid, norm, h, nb, structure="H", uplo=uplo)
            for letter in alts:
                assert dlaf.pxlanhe(letter, uplo, n, h, 1, 1, desc) == want, (norm, letter, uplo)
            for diag in "NU":
                want = dlaf.matrix_norm(grid, norm, a, nb, structure="T", uplo=uplo, diag=diag)
                for letter in alts:
                    assert dlaf.pxlantr(letter, uplo.lower(), diag.lower(), n, a, 1, 1, desc) == want, (norm, letter)
    # a rectangular p?lange
    m2, n2 = 130, 67
    r = exact_operand(t, m2, n2, False)
    for norm in NORMS:
        assert dlaf.pxlange(norm, m2, n2, r, 1, 1, [1, grid.context, m2, n2, nb, nb, 0, 0, m2]) == \
            dlaf.matrix_norm(grid, norm, r, nb)


# ---------------------------------------------------------------------------------------------------- (9) profile
def test_norm_profile_reports_the_referenced_tiles(dlaf, grid):
    n, nb = 1100, 256
    a = uniform_operand("d", n, n)
    ext = [min(nb, n - k * nb) for k in range(-(-n // nb))]
    full = sum(r * c for r in ext for c in ext) * 8
    lower = sum(ext[i] * ext[j] for i in range(len(ext)) for j in range(i + 1)) * 8
    assert full == n * n * 8
    for norm in NORMS:
        dlaf.matrix_norm(grid, norm, a, nb)
        ms, by = dlaf.norm_profile()
        assert ms > 0 and by == full, (norm, ms, by)
        for structure in "HT":
            dlaf.matrix_norm(grid, norm, a, nb, structure=structure, uplo="L")
            ms, by = dlaf.norm_profile()
            assert ms > 0 and by == lower, (norm, structure, ms, by)
    assert 0.5 < lower / full < 0.65
