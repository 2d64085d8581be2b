"""CPU tests of the long-double checkers of band -> tridiagonal in oracle/tridiag.py (b2t_backward_error,
b2t_reflector_unitarity, b2t_layout, b2t_spectrum): each accepts the fp64 restatement of the reference's bulge chase and
flags the corruptions it exists for -- a tau perturbed by 1e-6 relative, a stray nonzero outside the reflector slots, a
swapped pair of diagonal entries, a NaN."""
import numpy as np
import pytest

from oracle import tridiag as td

CASES = [(np.float64, 40, 4), (np.float64, 37, 3), (np.complex128, 34, 6), (np.complex128, 25, 2), (np.float64, 20, 19)]


def band_of(n, band, dt, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n))
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.uniform(-1, 1, (n, n))
    a = np.tril(a)
    a = a + np.tril(a, -1).conj().T
    a[np.arange(n), np.arange(n)] = a.diagonal().real
    i, j = np.indices((n, n))
    a[np.abs(i - j) > band] = 0
    return a.astype(dt)


@pytest.fixture(params=CASES, ids=lambda c: f"{np.dtype(c[0]).char}-{c[1]}-{c[2]}")
def reduced(request):
    dt, n, band = request.param
    a = band_of(n, band, dt, n + band)
    d, e, v = td.band_to_tridiag(a, band)
    return a, band, d, e, v


def ok(r):
    return r[0] <= 1


def test_checkers_accept_the_restatement(reduced):
    a, band, d, e, v = reduced
    checks = td.b2t_checks(a, band, d, e, v)
    assert not td.b2t_failures(checks), checks
    # well inside their bars, not at their edge
    assert checks["backward"][0] < 0.2 and checks["spectrum"][0] < 0.5 and checks["layout"][0] == 0, checks


def test_checkers_hold_every_scale(reduced):
    """no absolute floor: the restatement of 2^j A is 2^j times that of A and passes at any j"""
    a, band, d, e, v = reduced
    for j in (-900, 900):
        checks = td.b2t_checks(np.ldexp(a.real, j) + (1j * np.ldexp(a.imag, j) if np.iscomplexobj(a) else 0), band,
                               np.ldexp(d, j), np.ldexp(e, j), v)
        assert not td.b2t_failures(checks), (j, checks)
    # ... and a tiny matrix is not let through because it is tiny
    checks = td.b2t_checks(a * 1e-200, band, d * 1e-200, e * 1e-200 * 1.01, v)
    assert not ok(checks["backward"]) and not ok(checks["spectrum"]), checks


def test_perturbed_tau_is_flagged(reduced):
    a, band, d, e, v = reduced
    refl = td.reflector_list(a.shape[0], band, a.dtype)
    taus = [(sw, st, pos) for sw, st, first, size, pos in refl if v[pos, sw] != 0]
    sw, st, pos = taus[len(taus) // 2]
    w = v.copy()
    w[pos, sw] *= 1 + 1e-6
    assert not ok(td.b2t_backward_error(a, band, d, e, w))
    r = td.b2t_reflector_unitarity(w, band)
    assert not ok(r) and r[1] == f"(sweep {sw}, step {st})", r
    assert ok(td.b2t_layout(w, band, d, e))


def test_stray_nonzero_is_flagged(reduced):
    a, band, d, e, v = reduced
    n = a.shape[0]
    slot = np.zeros((n, n), dtype=bool)
    for sw, st, first, size, pos in td.reflector_list(n, band, a.dtype):
        slot[pos:pos + size, sw] = True
    free = np.argwhere(~slot)
    for r, c in (free[0], free[len(free) // 2], free[-1]):
        w = v.copy()
        w[r, c] = 1e-300
        assert not ok(td.b2t_layout(w, band, d, e)), (r, c)


def test_swapped_diagonal_is_flagged(reduced):
    a, band, d, e, v = reduced
    i = int(np.argmax(np.abs(np.diff(d))))
    dd = d.copy()
    dd[[i, i + 1]] = dd[[i + 1, i]]
    assert not ok(td.b2t_backward_error(a, band, dd, e, v))
    assert not ok(td.b2t_spectrum(a, band, dd, e))


def test_nan_is_flagged(reduced):
    a, band, d, e, v = reduced
    dn = d.copy()
    dn[len(d) // 2] = np.nan
    en = e.copy()
    en[-1] = np.nan
    for dd, ee in ((dn, e), (d, en)):
        for r in (td.b2t_backward_error(a, band, dd, ee, v), td.b2t_layout(v, band, dd, ee), td.b2t_spectrum(a, band, dd, ee)):
            assert not ok(r) and np.isnan(r[0]), r
    sw, st, first, size, pos = td.reflector_list(a.shape[0], band, a.dtype)[0]
    w = v.copy()
    w[pos + size - 1, sw] = np.nan
    for r in (td.b2t_backward_error(a, band, d, e, w), td.b2t_reflector_unitarity(w, band), td.b2t_layout(w, band, d, e)):
        assert not ok(r), r


def test_spectrum_beyond_the_long_double_size_uses_lapack():
    """above sturm_max the spectrum of T comes from LAPACK on T / 2^k: same verdicts"""
    a = band_of(60, 5, np.float64, 1)
    d, e, v = td.band_to_tridiag(a, 5)
    assert td.b2t_spectrum(a, 5, d, e, sturm_max=10)[0] < 0.5
    dd = d.copy()
    dd[3] += 1e-9
    assert not ok(td.b2t_spectrum(a, 5, dd, e, sturm_max=10))


def test_zero_band_passes():
    n, band = 12, 3
    a = np.zeros((n, n))
    d, e, v = td.band_to_tridiag(a, band)
    checks = td.b2t_checks(a, band, d, e, v)
    assert all(r[0] == 0 for r in checks.values()), checks
