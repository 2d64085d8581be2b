"""GPU tests of the partial-spectrum entries (a range [begin, end) of eigenvalue indices) on one process: the
tridiagonal solver, hermitian_eigensolver, hermitian_generalized_eigensolver and the ScaLAPACK-like entries.

Bars: the three conditions of the reference's test_eigensolver_correctness.h as oracle/tridiag.py::check_eigensolver
restates them, restated here once more for an n x k block of columns with m = n (check_eigensolver compares against
np.eye(m), which needs a square Z): orth = max|Z^H Z - I_k| <= 10 n error, elementwise |A z_j - w[begin + j] z_j| <=
2 n error absolute or relative to |w z|, w ascending.  They are elementwise subsets of what the full solver meets on the
same inputs.  Beside them: w is bit-identical to the full call's, every element of a sentinel-filled store outside the
wanted columns stays bit-identical (a padded ld, rows above and below, columns left and right), and the range [0, n)
through the new entry gives the bits of the old entry.

The tridiagonal solver's eigenvectors are also compared with the full call's columns: |z_ranged - z_full[:, begin:end]|
<= 2 n eps elementwise.  Only the root product may differ between the two calls, and only in its column tiling; each of
its elements is an inner product of a row of Q and a column of U (2-norms <= 1 and ~ 1), so each computation is within
gamma_n of the exact value."""
import functools

import numpy as np
import pytest

from oracle import tridiag as td

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
SENT = -3.25


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
    yield lambda b_min: dlaf.eigensolver_min_band(b_min)
    dlaf.eigensolver_min_band(old)


def clamp(ranges, n):
    """the ranges of a case, each clamped into [0, n] (a size smaller than the block keeps every case), without repeats"""
    out = []
    for b, e in ranges:
        e = min(max(e, 0), n)
        b = min(max(b, 0), e)
        if (b, e) not in out:
            out.append((b, e))
    return out


def check_block(what, a_full, w, zk, begin, dt, b_full=None):
    """the three conditions of check_eigensolver on the n x k block zk = the eigenvectors of w[begin : begin + k]"""
    n, k = a_full.shape[0], zk.shape[1]
    err = td.error_of(dt)
    assert zk.shape[0] == n and np.all(np.diff(w) >= 0), (what, "eigenvalues not ascending")
    g = zk.conj().T @ zk
    orth = float(np.abs(g - np.eye(k)).max(initial=0))
    el = zk * w[None, begin:begin + k]
    diff = np.abs(a_full @ zk - el)
    tol = 2 * n * err
    res_ok = bool(np.all((diff <= tol) | (diff <= tol * np.abs(el))))
    print(f"RATIO {what} [{begin},{begin + k}) orth={orth / (10 * n * err):.3g} residual={float(diff.max(initial=0)) / tol:.3g}")
    assert orth <= 10 * n * err, (what, begin, k, orth, 10 * n * err)
    assert res_ok, (what, begin, k, float(diff.max(initial=0)), tol)


def store_for(n, ncols, dt, top=3, bottom=4, left=2, right=2):
    """a sentinel-filled column-major store with the n x ncols matrix inside it: padded ld, sentinel rows above and below,
    sentinel columns left and right"""
    store = np.full((n + top + bottom, ncols + left + right), SENT, dtype=dt, order="F")
    return store, store[top:top + n, left:left + ncols]


def untouched_outside(store, view_cols, n, top=3, left=2):
    """every element of the store outside rows [top, top + n) x the given columns of the view is still the sentinel"""
    mask = np.ones(store.shape, dtype=bool)
    b, e = view_cols
    mask[top:top + n, left + b:left + e] = False
    return bool(np.all(store[mask] == np.dtype(store.dtype).type(SENT)))


# ------------------------------------------------------------------------------------------- tridiagonal solver
def tridiag_ranges(n):
    cand = [(0, 1), (0, n), (n - 1, n), (n // 3, n // 3 + 17), (5, n - 5), (n // 2, n // 2)]
    out = []
    for b, e in cand:
        if 0 <= b <= e <= n and (b, e) not in out:
            out.append((b, e))
    return out


def run_tridiag(dlaf, what, d, e, nb, dt):
    n = len(d)
    eps = float(np.finfo(dt).eps)
    w_full, z_full = dlaf.tridiagonal_eigensolver(d.copy(), e.copy(), nb)
    full = np.diag(d) + np.diag(e, -1) + np.diag(e, 1)
    for begin, end in tridiag_ranges(n):
        k = end - begin
        store, z = store_for(n, k, dt)
        w, _ = dlaf.tridiagonal_eigensolver(d.copy(), e.copy(), nb, eigenvalues_index=(begin, end), z=z)
        assert np.array_equal(w, w_full), (what, begin, end, "w differs from the full call")
        assert untouched_outside(store, (0, k), n), (what, begin, end, "sentinel overwritten")
        check_block(what, full, w, z, begin, dt)
        dz = float(np.abs(z - z_full[:, begin:end]).max(initial=0))
        print(f"RATIO {what} [{begin},{end}) |z - z_full|={dz / (2 * n * eps):.3g}")
        assert dz <= 2 * n * eps, (what, begin, end, dz, 2 * n * eps)
        if (begin, end) == (0, n):
            assert np.array_equal(z, z_full), (what, "[0, n) through the new entry differs from the old entry")


@pytest.mark.parametrize("t", ["d", "s"])
def test_tridiagonal_random(dlaf, t):
    """a single leaf (1, 64), one merge (65, 130), roots narrower and wider than 16 columns, several levels (515)"""
    dt = DT[t]
    for n, nb in [(1, 8), (64, 64), (65, 32), (130, 64), (515, 128)]:
        rng = np.random.default_rng(n + 1)
        d = rng.uniform(-1, 1, n).astype(dt)
        e = rng.uniform(-1, 1, max(n - 1, 0)).astype(dt)
        run_tridiag(dlaf, f"tridiag {t} n={n}", d, e, nb, dt)


def deflation_heavy(n=600):
    cases = []
    cases.append((np.ones(n), np.full(n - 1, 1e-14)))
    w21 = np.abs(np.arange(-10, 11)).astype(np.float64)
    d = np.tile(w21, 20)
    e = np.ones(d.size - 1)
    e[20::21] = 1e-11
    cases.append((d[:n], e[:n - 1]))
    d = np.zeros(n)
    e = np.ones(n - 1)
    e[63::64] = 0.0
    cases.append((d, e))
    return cases


@pytest.mark.parametrize("t", ["d", "s"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_tridiagonal_deflation_heavy(dlaf, t, which):
    """matrices that deflate almost everything at the root: the wanted range straddles the deflated and the non-deflated
    runs of columns"""
    dt = DT[t]
    d, e = deflation_heavy()[which]
    run_tridiag(dlaf, f"tridiag {t} deflation {which}", d.astype(dt), e.astype(dt), 128, dt)


# -------------------------------------------------------------------------------------------------- eigensolver
def random_hermitian(n, dt, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n)).astype(dt)
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.uniform(-1, 1, (n, n)).astype(dt)
    return np.asfortranarray((a + a.conj().T).astype(dt))


def eig_ranges(n, nb):
    return clamp([(0, 1), (0, nb), (0, nb + 1), (nb + 3, min(n, 2 * nb + 5)), (n - 1, n), (n // 2, n // 2), (0, n)], n)


def run_eigensolver(dlaf, grid, what, a0, nb, dt):
    n = a0.shape[0]
    w_full, z_full = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb)
    for begin, end in eig_ranges(n, nb):
        store, z = store_for(n, n, dt)
        a = a0.copy(order="F")
        a[np.triu_indices(n, 1)] = -9.9
        w, _ = dlaf.hermitian_eigensolver(grid, "L", a, nb, eigenvalues_index=(begin, end), z=z)
        assert np.array_equal(w, w_full), (what, begin, end, "w differs from the full call")
        assert untouched_outside(store, (begin, end), n), (what, begin, end, "sentinel overwritten")
        check_block(what, a0, w, z[:, begin:end], begin, dt)
        if (begin, end) == (0, n):
            assert np.array_equal(z, z_full), (what, "[0, n) through the new entry differs from the old entry")


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_eigensolver_small(dlaf, grid, min_band, t):
    """sizes of the reference's test_eigensolver.cpp: smaller than a block, ragged tiles, the two sub-band cases"""
    dt = DT[t]
    for n, nb, b_min in [(5, 8, 100), (34, 13, 100), (32, 6, 3), (34, 8, 3)]:
        min_band(b_min)
        run_eigensolver(dlaf, grid, f"eig {t} n={n} nb={nb} min_band={b_min}", random_hermitian(n, dt, 11 + n), nb, dt)


@pytest.mark.parametrize("t,n,nb", [("d", 1100, 256), ("z", 700, 128)])
def test_eigensolver_band_128(dlaf, grid, t, n, nb):
    """band 128: the fused back-transformation (d) on a narrow operand, several tree levels in the tridiagonal solver"""
    dt = DT[t]
    run_eigensolver(dlaf, grid, f"eig {t} n={n} nb={nb}", random_hermitian(n, dt, 3), nb, dt)


def test_eigensolver_identity(dlaf, grid, min_band):
    """the identity: everything deflates, every reflector is zero"""
    n, nb = 34, 8
    min_band(4)
    for t in "sdcz":
        dt = DT[t]
        a0 = np.asfortranarray(np.eye(n, dtype=dt))
        run_eigensolver(dlaf, grid, f"eig {t} identity", a0, nb, dt)
        w, _ = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb, eigenvalues_index=(3, 9))
        assert np.all(w == 1), (t, w)


# -------------------------------------------------------------------------------------------------- generalized
@pytest.mark.parametrize("t", ["d", "z"])
@pytest.mark.parametrize("n,nb", [(34, 8), (300, 64)])
def test_generalized(dlaf, grid, t, n, nb):
    """B-orthonormality and A Z = B Z Lambda on the k columns with test_gen_eigensolver.cpp's bars, plain and
    `_factorized`"""
    dt = DT[t]
    err = td.error_of(dt)
    a0 = random_hermitian(n, dt, 21 + n)
    b0 = random_hermitian(n, dt, 22 + n)
    b0 = np.asfortranarray(b0 @ b0.conj().T / n + np.eye(n, dtype=dt) * 2)
    bf = b0.copy(order="F")
    w_full, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bf, nb)   # bf <- the factor of B
    wf_full, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), bf.copy(order="F"), nb, factorized=True)
    for factorized in (False, True):
        for begin, end in clamp([(0, n // 4), (nb + 3, 2 * nb + 5)], n):
            k = end - begin
            store, z = store_for(n, n, dt)
            b = (bf if factorized else b0).copy(order="F")
            w, _ = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), b, nb, factorized=factorized,
                                                          eigenvalues_index=(begin, end), z=z)
            what = (t, n, nb, begin, end, factorized)
            assert np.array_equal(w, wf_full if factorized else w_full), (what, "w differs from the full call")
            assert untouched_outside(store, (begin, end), n), (what, "sentinel overwritten")
            if not factorized:
                assert np.array_equal(np.tril(b), np.tril(bf)), (what, "B is not the factor the full call leaves")
            zk = z[:, begin:end]
            assert np.all(np.diff(w) >= 0)
            orth = float(np.abs(zk.conj().T @ b0 @ zk - np.eye(k)).max())
            res = float(np.abs(a0 @ zk - (b0 @ zk) * w[None, begin:end]).max())
            obar = 10 * n * err * np.abs(b0).max()
            rbar = 10 * n * err * max(1.0, np.abs(a0).max() * np.abs(w).max())
            print(f"RATIO gen {what} orth={orth / obar:.3g} residual={res / rbar:.3g}")
            assert orth <= obar, (what, orth, obar)
            assert res <= rbar, (what, res, rbar)


# -------------------------------------------------------------------------------------- ScaLAPACK-like entries
@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_scalapack_like_entries(dlaf, grid, t):
    """dlaf_p?syevd_partial_spectrum / p?heevd_partial_spectrum with (il, iu) = (begin + 1, end): the bits of the context
    entry; (1, 0) is the empty range and leaves z untouched"""
    dt = DT[t]
    n, nb, begin, end = 34, 8, 11, 21
    a0 = random_hermitian(n, dt, 5)
    s_ref, z_ref = store_for(n, n, dt)
    w_ref, _ = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb, eigenvalues_index=(begin, end), z=z_ref)
    store, z = store_for(n, n, dt)
    ld = store.shape[0]
    desc = [1, grid.context, n, n, nb, nb, 0, 0, ld]
    a = a0.copy(order="F")
    w, info = dlaf.pxheevd_partial_spectrum("L", a, [1, grid.context, n, n, nb, nb, 0, 0, n], z, desc, begin + 1, end, n)
    assert info == 0
    assert np.array_equal(w, w_ref) and np.array_equal(store, s_ref), (t, "differs from the context entry")
    check_block(f"p{t}(sy|he)evd", a0, w, z[:, begin:end], begin, dt)
    store, z = store_for(n, n, dt)
    w, info = dlaf.pxheevd_partial_spectrum("L", a0.copy(order="F"), [1, grid.context, n, n, nb, nb, 0, 0, n], z, desc, 1, 0, n)
    assert info == 0 and np.array_equal(w, w_ref) and np.all(store == dt(SENT)), (t, "the empty range wrote to z")
