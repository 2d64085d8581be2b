"""GPU tests, one process, of the eigenvalues-only entries (hermitian_eigenvalues, hermitian_generalized_eigenvalues, the
ScaLAPACK-like forms) and of the partial spectrum selected by value (eigenvalues_value=(vl, vu)), s / d / c / z.

Matrices: A = Q diag(lambda) Q^H with a prescribed spectrum in four groups separated by gaps of more than 1, so that an
interval boundary put into a gap selects a known index range whatever the rounding.  Generalized problems: B = L L^H
with a random well-conditioned L and A = L (Q diag(lambda) Q^H) L^H, which has the same prescribed eigenvalues.

Bar for eigenvalues-only against the eigensolver's w on a copy: the one tests/test_gpu_eigensolver.py holds the
eigensolver's w to against numpy, unchanged: max |w - w_ref| <= n error max |w_ref|, error = 2 eps.  Both calls run the
same deterministic reductions, so they differ in the tridiagonal stage alone (bisection / divide & conquer).
By value, everything is bit for bit: w against the full call's, z (the whole sentinel-filled store) against the
eigenvalues_index call the interval resolves to."""
import functools

import numpy as np
import pytest

from oracle import tridiag as td

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
SENT = -3.25
SHAPES = [(1, 64), (1, 128), (130, 64), (130, 128), (400, 64), (400, 128), (400, 256)]   # (400, 256): band 128 at nb = 256


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def spectrum(n):
    """four groups, each within [2 g + 1, 2 g + 2), g = 0 .. 3: gaps of more than 1 around 2.5, 4.5, 6.5"""
    q = max((n + 3) // 4, 1)
    i = np.arange(n)
    return 1.0 + (i // q) * 2.0 + (i % q) / q


@functools.lru_cache(maxsize=None)
def problem(n, t, generalized=False):
    """(A, B or None, lambda): read-only, shared"""
    dt = DT[t]
    wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    rng = np.random.default_rng(1000 * n + ord(t))

    def rnd(*shape):
        x = rng.standard_normal(shape)
        return x + 1j * rng.standard_normal(shape) if wide is np.complex128 else x

    lam = spectrum(n)
    q, _ = np.linalg.qr(rnd(n, n))
    m = (q * lam[None, :]) @ q.conj().T
    b = None
    if generalized:
        l = np.tril(rnd(n, n)) / np.sqrt(n) + 2 * np.eye(n)
        m = l @ m @ l.conj().T
        b = np.asfortranarray((l @ l.conj().T).astype(dt))
        b.flags.writeable = False
    a = np.asfortranarray(((m + m.conj().T) / 2).astype(dt))
    a.flags.writeable = False
    return a, b, lam


def close(what, w, w_ref, n, dt):
    bar = n * td.error_of(dt) * np.abs(w_ref).max()
    diff = float(np.abs(w - w_ref).max(initial=0))
    print(f"RATIO {what} |w - w_eigensolver| / (n error max|w|) = {diff / bar if bar else 0:.3g}")
    assert diff <= bar, (what, diff, bar)


def ranges(n):
    cand = [(0, n), (0, 1), (n - 1, n), (n // 3, n // 3 + 70), (0, 0), (n // 2, n // 2), (n, n)]
    out = []
    for b, e in cand:
        e = min(e, n)
        if 0 <= b <= e and (b, e) not in out:
            out.append((b, e))
    return out


# ------------------------------------------------------------------------------------------------ eigenvalues only
@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_eigenvalues_only(dlaf, grid, t):
    dt = DT[t]
    rt = np.zeros(0, dtype=dt).real.dtype
    for n, nb in SHAPES:
        a0, _, lam = problem(n, t)
        what = f"eigenvalues {t} n={n} nb={nb}"
        w_ref, _ = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb)
        a = a0.copy(order="F")
        a[np.triu_indices(n, 1)] = -9.9
        kept = a.copy(order="F")
        w = dlaf.hermitian_eigenvalues(grid, "L", a, nb)
        prof = dlaf.eigensolver_profile()
        assert prof[3:5] == [0, 0] and prof[2] > 0, (what, prof)
        assert np.array_equal(a, kept), (what, "a was written")
        assert w.dtype == rt and np.all(np.diff(w) >= 0), what
        close(what, w, w_ref, n, dt)
        for b, e in ranges(n):
            out = np.full(n, SENT, dtype=rt)
            r = dlaf.hermitian_eigenvalues(grid, "L", a0.copy(order="F"), nb, eigenvalues_index=(b, e), w=out)
            assert r is out and np.array_equal(out[b:e], w[b:e]), (what, b, e, "differs from the full call's slice")
            assert np.all(out[:b] == rt.type(SENT)) and np.all(out[e:] == rt.type(SENT)), (what, b, e, "sentinel overwritten")
            assert dlaf.eigensolver_profile()[3:5] == [0, 0]


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_generalized_eigenvalues_only(dlaf, grid, t):
    dt = DT[t]
    rt = np.zeros(0, dtype=dt).real.dtype
    for n, nb in [(130, 64), (400, 128)]:
        a0, b0, lam = problem(n, t, True)
        what = f"generalized eigenvalues {t} n={n} nb={nb}"
        bf = b0.copy(order="F")
        w_ref, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bf, nb)        # bf <- factor
        b = b0.copy(order="F")
        w = dlaf.hermitian_generalized_eigenvalues(grid, "L", a0.copy(order="F"), b, nb)
        assert dlaf.eigensolver_profile()[3:5] == [0, 0]
        assert np.array_equal(np.tril(b), np.tril(bf)), (what, "b is not the factor the eigensolver leaves")
        close(what, w, w_ref, n, dt)
        wf_ref, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bf.copy(order="F"), nb, factorized=True)
        b = bf.copy(order="F")
        wf = dlaf.hermitian_generalized_eigenvalues(grid, "L", a0.copy(order="F"), b, nb, factorized=True)
        assert np.array_equal(b, bf), (what, "the factor was written")
        close(what + " factorized", wf, wf_ref, n, dt)
        lo, hi = n // 3, n // 3 + 70
        for factorized in (False, True):
            out = np.full(n, SENT, dtype=rt)
            dlaf.hermitian_generalized_eigenvalues(grid, "L", a0.copy(order="F"), (bf if factorized else b0).copy(order="F"), nb,
                                                   factorized=factorized, eigenvalues_index=(lo, hi), w=out)
            assert np.array_equal(out[lo:hi], (wf if factorized else w)[lo:hi]), (what, factorized)
            assert np.all(out[:lo] == rt.type(SENT)) and np.all(out[hi:] == rt.type(SENT)), (what, factorized)


# ------------------------------------------------------------------------------------------------ by value
def intervals(lam):
    """(vl, vu) with both ends in gaps of the spectrum: below it, above it, around all of it, nothing between two
    eigenvalues, a proper part, and vl >= vu"""
    lo, hi = float(lam.min()), float(lam.max())
    out = [(lo - 3, lo - 1), (hi + 1, hi + 3), (lo - 1, hi + 1), (2.25, 2.75), (2.5, 6.5), (4.5, 2.5), (4.5, 4.5)]
    return [(vl, vu, int((lam <= vl).sum()), int((lam <= vu).sum()) if vl < vu else int((lam <= vl).sum())) for vl, vu in out]


def store_for(n, dt):
    store = np.full((n + 7, n + 4), SENT, dtype=dt, order="F")
    return store, store[3:3 + n, 2:2 + n]


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_partial_spectrum_by_value(dlaf, grid, t):
    dt = DT[t]
    for n, nb in [(1, 64), (1, 128), (130, 64), (400, 128), (400, 256)]:
        a0, _, lam = problem(n, t)
        w_full, _ = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb)
        for vl, vu, begin, end in intervals(lam):
            what = f"by value {t} n={n} nb={nb} ({vl}, {vu}]"
            store, z = store_for(n, dt)
            w, _, found = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb, eigenvalues_value=(vl, vu), z=z)
            assert found == (begin, end), (what, found, (begin, end))
            assert np.array_equal(w, w_full), (what, "w differs from the full call")
            store_ref, z_ref = store_for(n, dt)
            dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb, eigenvalues_index=(begin, end), z=z_ref)
            assert np.array_equal(store, store_ref), (what, "z differs from the index-range call")
            mask = np.ones(store.shape, dtype=bool)
            mask[3:3 + n, 2 + begin:2 + end] = False
            assert np.all(store[mask] == dt(SENT)), (what, "sentinel overwritten")
            assert not np.any(z[:, begin:end] == dt(SENT)), (what, "wanted columns not written")


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_generalized_partial_spectrum_by_value(dlaf, grid, t):
    dt = DT[t]
    n, nb = 130, 64
    a0, b0, lam = problem(n, t, True)
    bf = b0.copy(order="F")
    w_full, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bf, nb)
    for factorized in (False, True):
        for vl, vu, begin, end in intervals(lam)[3:6]:
            what = f"generalized by value {t} factorized={factorized} ({vl}, {vu}]"
            bsrc = bf if factorized else b0
            store, z = store_for(n, dt)
            w, _, found = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bsrc.copy(order="F"), nb,
                                                                 factorized=factorized, eigenvalues_value=(vl, vu), z=z)
            assert found == (begin, end), (what, found, (begin, end))
            store_ref, z_ref = store_for(n, dt)
            w_ref, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bsrc.copy(order="F"), nb,
                                                              factorized=factorized, eigenvalues_index=(begin, end), z=z_ref)
            assert np.array_equal(w, w_ref), (what, "w differs from the index-range call")
            if not factorized:
                assert np.array_equal(w, w_full), (what, "w differs from the full call")
            assert np.array_equal(store, store_ref), (what, "z differs from the index-range call")


def test_selections_are_mutually_exclusive(dlaf, grid):
    a0, _, _ = problem(130, "d")
    with pytest.raises(ValueError):
        dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), 64, eigenvalues_index=(0, 3), eigenvalues_value=(0.0, 1.0))


# ------------------------------------------------------------------------------------------------ ScaLAPACK-like
@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_scalapack_like_entries(dlaf, grid, t):
    """dlaf_p?syevd_eigenvalues / p?heevd_eigenvalues with (il, iu) and *_partial_spectrum_by_value with vl, vu, m"""
    dt = DT[t]
    rt = np.zeros(0, dtype=dt).real.dtype
    n, nb = 130, 64
    a0, _, lam = problem(n, t)
    desc = [1, grid.context, n, n, nb, nb, 0, 0, n]
    w_only = dlaf.hermitian_eigenvalues(grid, "L", a0.copy(order="F"), nb)
    out = np.full(n, SENT, dtype=rt)
    w, info = dlaf.pxheevd_eigenvalues("L", a0.copy(order="F"), desc, 12, 40, n, w=out)
    assert info == 0 and w is out
    assert np.array_equal(out[11:40], w_only[11:40]) and np.all(out[:11] == rt.type(SENT)) and np.all(out[40:] == rt.type(SENT))
    vl, vu, begin, end = intervals(lam)[4]
    store, z = store_for(n, dt)
    descz = [1, grid.context, n, n, nb, nb, 0, 0, store.shape[0]]
    w, m, info = dlaf.pxheevd_partial_spectrum_by_value("L", a0.copy(order="F"), desc, z, descz, vl, vu, n)
    assert info == 0 and m == end - begin, (t, m, info, begin, end)
    store_ref, z_ref = store_for(n, dt)
    w_ref, _ = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb, eigenvalues_index=(begin, end), z=z_ref)
    assert np.array_equal(w, w_ref) and np.array_equal(store, store_ref), (t, "differs from the context entry")


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_scalapack_like_generalized_entries(dlaf, grid, t):
    """dlaf_p?sygvd_eigenvalues[_factorized] / p?hegvd_eigenvalues[_factorized] and the *_partial_spectrum_by_value forms
    of the generalized problem, each once: the bits of the context entries, m and info == 0"""
    dt = DT[t]
    rt = np.zeros(0, dtype=dt).real.dtype
    n, nb = 130, 64
    a0, b0, lam = problem(n, t, True)
    desc = [1, grid.context, n, n, nb, nb, 0, 0, n]
    bf = b0.copy(order="F")
    w_only = dlaf.hermitian_generalized_eigenvalues(grid, "L", a0.copy(order="F"), bf, nb)            # bf <- factor
    vl, vu, begin, end = intervals(lam)[4]
    for factorized in (False, True):
        bsrc = bf if factorized else b0
        out = np.full(n, SENT, dtype=rt)
        b = bsrc.copy(order="F")
        w, info = dlaf.pxhegvd_eigenvalues("L", a0.copy(order="F"), desc, b, desc, 12, 40, n, factorized=factorized, w=out)
        assert info == 0 and w is out, (t, factorized, info)
        assert np.array_equal(out[11:40], w_only[11:40]), (t, factorized, "differs from the context entry")
        assert np.all(out[:11] == rt.type(SENT)) and np.all(out[40:] == rt.type(SENT)), (t, factorized)
        assert np.array_equal(np.tril(b), np.tril(bf)), (t, factorized, "b is not the factor")
        store, z = store_for(n, dt)
        descz = [1, grid.context, n, n, nb, nb, 0, 0, store.shape[0]]
        w, m, info = dlaf.pxhegvd_partial_spectrum_by_value("L", a0.copy(order="F"), desc, bsrc.copy(order="F"), desc, z, descz,
                                                            vl, vu, n, factorized=factorized)
        assert info == 0 and m == end - begin, (t, factorized, m, info, begin, end)
        store_ref, z_ref = store_for(n, dt)
        w_ref, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bsrc.copy(order="F"), nb,
                                                          factorized=factorized, eigenvalues_index=(begin, end), z=z_ref)
        assert np.array_equal(w, w_ref) and np.array_equal(store, store_ref), (t, factorized, "differs from the context entry")
