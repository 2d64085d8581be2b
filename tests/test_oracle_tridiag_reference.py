"""CPU tests pinning the extended-precision reference of the tridiagonal eigensolver tests (oracle/tridiag.py:
sturm_eigvals, check_tridiag_solution, tridiag_family): every family against mpmath.eigsy at 40 digits on the exact
inputs, closed-form spectra (1D Laplacian, the free chain d = 0 / e = 1, Clement), fp32 inputs as well as fp64, and
the checker's findings on solutions that are known to be right or wrong."""
import mpmath
import numpy as np
import pytest
import scipy.linalg as sl

from oracle import tridiag as td

LD_EPS = float(np.finfo(np.longdouble).eps)


def mp_eigvals(d, e):
    """mpmath.eigsy at 40 digits on the exact (binary) inputs, as float64 pairs (hi, lo): hi + lo carries ~32 digits"""
    n = len(d)
    with mpmath.workdps(40):
        a = mpmath.zeros(n, n)
        for i in range(n):
            a[i, i] = mpmath.mpf(float(d[i]))
        for i in range(n - 1):
            a[i, i + 1] = a[i + 1, i] = mpmath.mpf(float(e[i]))
        ev = sorted(mpmath.eigsy(a, eigvals_only=True)) if n > 1 else [a[0, 0]]
        hi = np.array([float(v) for v in ev])
        lo = np.array([float(v - mpmath.mpf(h)) for v, h in zip(ev, hi)])
    return hi, lo


def test_long_double_is_extended():
    assert LD_EPS < 1e-18


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("family", td.FAMILIES)
def test_sturm_matches_mpmath(family, dt):
    """the Sturm-count bisection agrees with a 40-digit eigensolver to a few long-double units of |T|: ~1e-3 eps of
    fp64, far below any bar it referees"""
    for n in (1, 2, 3, 40):
        d, e = td.tridiag_family(family, n, dt, seed=1)
        assert d.dtype == dt and e.dtype == dt and d.shape == (n,) and e.shape == (n - 1,)
        w = td.sturm_eigvals(d, e)
        hi, lo = mp_eigvals(d, e)
        ref = hi.astype(np.longdouble) + lo.astype(np.longdouble)
        norm = float(np.abs(ref).max())
        err = float(np.abs(w - ref).max())
        assert err <= 8 * n * LD_EPS * norm, (family, n, err / (LD_EPS * max(norm, 1e-300)))
        assert np.all(np.diff(w) >= 0)
        if norm > 0:
            # rounded to fp64 it is mpmath's result rounded to fp64 up to one unit of |T|'s last place
            assert np.abs(w.astype(np.float64) - hi).max() <= np.finfo(np.float64).eps * norm, (family, n)


def test_family_exact_structure():
    for dt in (np.float64, np.float32):
        for n in (1, 2, 3, 63, 64, 65, 129, 200):
            d, e = td.tridiag_family("zero", n, dt)
            assert not d.any() and not e.any()
            d, e = td.tridiag_family("const", n, dt)
            assert np.all(d == d[0]) and not e.any()
            assert np.all(td.sturm_eigvals(d, e) == np.longdouble(d[0]))
            d, e = td.tridiag_family("diag", n, dt)
            assert np.unique(d).size == n and not e.any()
            assert np.array_equal(td.sturm_eigvals(d, e), np.sort(d).astype(np.longdouble))
            d, e = td.tridiag_family("rho0", n, dt)
            assert not e[td.LEAF - 1::td.LEAF].any() and np.all(np.delete(e, np.arange(td.LEAF - 1, n - 1, td.LEAF)) != 0)
            d, e = td.tridiag_family("zero_e_inside", n, dt)
            assert np.all(e[td.LEAF - 1::td.LEAF] != 0) and (n < 12 or not e[10])
            d, e = td.tridiag_family("repeated", n, dt)
            if n >= 2 * td.LEAF:
                assert np.array_equal(d[:td.LEAF], d[td.LEAF:2 * td.LEAF])
            d, e = td.tridiag_family("graded", n, dt)
            assert np.all(d > 0) and d.min() >= np.finfo(dt).tiny and np.all(e >= np.finfo(dt).tiny)
            for s in ("neg", "alt", "mixed"):
                d, e = td.tridiag_family("rand_" + s, n, dt)
                if n > 3:
                    assert {"neg": np.all(e < 0), "alt": np.all(e[::2] > 0) and np.all(e[1::2] < 0),
                            "mixed": (e < 0).any() and (e > 0).any()}[s]
        # deterministic
        a, b = td.tridiag_family("dlatms_c", 65, dt, seed=3), td.tridiag_family("dlatms_c", 65, dt, seed=3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("mode", "abcde")
def test_dlatms_spectra(mode):
    """the tridiagonal matrix keeps the prescribed spectrum (fp64 reduction) and its condition number 1/eps"""
    n = 65
    d, e = td.tridiag_family("dlatms_" + mode, n, np.float64, seed=2)
    w = np.sort(np.abs(td.sturm_eigvals(d, e).astype(np.float64)))
    tol = 100 * n * np.finfo(np.float64).eps
    if mode == "e":  # log-uniform in [1/kappa, 1]
        assert w[-1] <= 1 + tol and w[0] >= np.finfo(np.float64).eps * (1 - tol) and w[-1] / w[0] > 1e6
        return
    assert abs(w[-1] - 1) <= tol
    assert w[0] <= 1e-12
    if mode == "a":
        assert np.sum(w > 0.5) == 1
    if mode == "b":
        assert np.sum(w < 0.5) == 1


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_sturm_closed_forms(dt):
    ld = np.longdouble
    for n in (1, 2, 3, 17, 64, 129):
        k = np.arange(1, n + 1, dtype=ld)
        c = np.cos(k * (4 * np.arctan(ld(1))) / (n + 1))
        # 1D Laplacian (exact in any type): 2 - 2 cos(k pi / (n + 1))
        d, e = np.full(n, 2, dtype=dt), np.full(n - 1, -1, dtype=dt)
        want = np.sort(2 - 2 * c)
        assert np.abs(td.sturm_eigvals(d, e) - want).max() <= 8 * n * LD_EPS * 4, n
        # free chain d = 0, e = 1: 2 cos(k pi / (n + 1))
        d, e = np.zeros(n, dtype=dt), np.ones(n - 1, dtype=dt)
        assert np.abs(td.sturm_eigvals(d, e) - np.sort(2 * c)).max() <= 8 * n * LD_EPS * 2, n
        # Clement, e_i = sqrt(i (n - i)): +-(n - 1), +-(n - 3), ...  In long double to long-double accuracy; from the
        # family (rounded to dt) within the perturbation of the rounding, |dT| <= eps(dt) |T|
        i = np.arange(1, n, dtype=ld)
        want = -(n - 1) + 2 * np.arange(n, dtype=ld)
        got = td.sturm_eigvals(np.zeros(n, dtype=ld), np.sqrt(i * (n - i)))
        assert np.abs(got - want).max() <= 8 * n * LD_EPS * max(n - 1, 1), n
        d, e = td.tridiag_family("clement", n, dt)
        assert np.abs(td.sturm_eigvals(d, e) - want).max() <= 2 * np.finfo(dt).eps * max(n - 1, 1), n


def test_sturm_is_exact_under_powers_of_two():
    d, e = td.tridiag_family("rand_mixed", 65, np.float64)
    w = td.sturm_eigvals(d, e)
    for k in (-600, -1, 1, 600):
        assert np.array_equal(td.sturm_eigvals(np.ldexp(d, k), np.ldexp(e, k)), np.ldexp(w, k))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_check_tridiag_solution(dt):
    """LAPACK's stedc passes with its usual few-eps margins, in units relative to |T|; a perturbed eigenvalue, a
    perturbed eigenvector and a solution of the transposed order are flagged -- also at a scale of 2^-60, where an
    absolute bar would see nothing.  n = 300: the residual is computed in two chunks of columns"""
    n = 300
    d, e = td.tridiag_family("rand_mixed", n, dt)
    ref = td.sturm_eigvals(d, e)
    for k in (0, -60):
        ds, es, rs = np.ldexp(d, k), np.ldexp(e, k), np.ldexp(ref, k)
        w, z = sl.eigh_tridiagonal(ds, es, lapack_driver="stev")
        w, z = w.astype(dt), z.astype(dt)
        f = td.check_tridiag_solution(ds, es, w, z, dt, w_ref=rs)
        assert f["sorted"] and f["eig"] <= 2 * n and f["residual"] <= 4 * n and f["orth"] <= 20 * n, f
        assert f["norm"] == float(np.abs(rs).max())
        w2 = w.copy()
        w2[n // 2] += dt(100 * n * np.finfo(dt).eps * f["norm"])
        g = td.check_tridiag_solution(ds, es, w2, z, dt, w_ref=rs)
        assert g["eig"] > 2 * n and g["residual"] > 4 * n
        z2 = z.copy()
        z2[:, 7] += dt(100 * n * np.finfo(dt).eps) * z[:, 8]
        g = td.check_tridiag_solution(ds, es, w, z2, dt, w_ref=rs)
        assert g["orth"] > 20 * n
        assert not td.check_tridiag_solution(ds, es, w[::-1], z[:, ::-1], dt, w_ref=rs)["sorted"]
        # a NaN eigenvector (a secular root on a pole) is a residual and an orthogonality finding that fails its bar,
        # in any chunk of columns; a NaN eigenvalue is an eigenvalue finding and unsorted
        for c in (3, 255, 256, n - 1):
            z2 = z.copy()
            z2[5, c] = np.nan
            g = td.check_tridiag_solution(ds, es, w, z2, dt, w_ref=rs)
            assert not g["residual"] <= 4 * n and not g["orth"] <= 20 * n, (c, g)
        w2 = w.copy()
        w2[n // 3] = np.nan
        g = td.check_tridiag_solution(ds, es, w2, z, dt, w_ref=rs)
        assert not g["eig"] <= 2 * n and not g["residual"] <= 4 * n and not g["sorted"], g
    # the reference of the zero matrix is exactly zero and any nonzero answer is infinitely wrong
    d, e = td.tridiag_family("zero", 5, dt)
    assert not td.sturm_eigvals(d, e).any()
    f = td.check_tridiag_solution(d, e, np.zeros(5, dt), np.eye(5, dtype=dt), dt)
    assert f["eig"] == 0 and f["residual"] == 0 and f["orth"] == 0
    assert td.check_tridiag_solution(d, e, np.full(5, 1e-30, dt), np.eye(5, dtype=dt), dt)["eig"] > 1e100
