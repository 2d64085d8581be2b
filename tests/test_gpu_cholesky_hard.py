"""The Cholesky drivers on input that is not diagonally dominant: ill-conditioned and graded positive definite matrices,
exact scale equivariance, and matrices that are not positive definite (planted pivots, pivots that turn negative only
through the trailing updates, NaN and Inf), through cholesky_factorization, p?potrf, p?potrs, the resident handle and the
generalized eigensolver drivers.  Inputs, references and measures: tests/hard_spd.py; their CPU half: test_hard_spd.py.

Accuracy.  With eps of the working type and everything formed in the wide type (float64 / complex128 for s / c,
longdouble / clongdouble for d / z):
    normwise        max|A - Lh Lh^H| / (n eps max|A|)
    componentwise   max(|A - Lh Lh^H| / (|Lh||Lh|^H)) / (n eps)
    solve           max_j ||b_j - A x_j||_inf / ((||A||_inf ||x_j||_inf + ||b_j||_inf) n eps)
The bars are 4 x the worst value the working-precision LAPACK route (scipy 1.15.3 / OpenBLAS ?potrf, cho_solve, x86-64)
reaches on the same rounded inputs over the whole input set (hard_spd.calibrate(); the factor 4 as in
test_gpu_inverse.py: MFMA block accumulation orders the sums differently from LAPACK):

                         s        c        d        z
    factor, normwise     0.01317  0.01824  0.01623  0.01795     bars  0.05268  0.07296  0.06492  0.07180
    factor, componentw.  0.04460  0.05080  0.05634  0.04997     bars  0.17840  0.20320  0.22536  0.19988
    solve, backward         -        -     0.01004  0.008721    bars     -        -     0.04016  0.034884

Not positive definite.  The reference is hard_spd.unblocked_info: the textbook column Cholesky in the wide type, failing at
the first pivot that is <= 0 or NaN (LAPACK is no referee for NaN: OpenBLAS's dpotrf returns 0 on it).  Every finite case
is decisive (test_hard_spd.py): rounding cannot move the index.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hard_spd as h  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = ["classic", "early", "sidecar", "pairs"]


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


@pytest.fixture(params=SCHEDULES)
def schedule(request, monkeypatch):
    """the issue orders of the tile DAG; DLAF_MI355X_SCHEDULE is read at every factorization"""
    monkeypatch.setenv("DLAF_MI355X_SCHEDULE", request.param)
    return request.param


def desc_of(grid, m, n, nb, ld):
    return [1, grid.context, m, n, nb, nb, 0, 0, ld]


# ------------------------------------------------------------------------------------------ accuracy of the factor
def check_factor(dlaf, grid, name, t, n, nb, uplo, label=""):
    a0 = h.family(name, t, n)
    buf, a = h.padded(a0)
    buf0 = buf.copy()
    assert dlaf.cholesky_factorization(grid, uplo, a, nb) == 0
    assert h.untouched(buf, buf0, uplo)
    assert h.diagonal_ok(a)
    norm, comp = h.factor_ratios(t, a0, h.lower_of(a, uplo))
    print(f"RATIO factor {t} {name} n={n} nb={nb} {uplo} {label}: normwise {norm:.4f} componentwise {comp:.4f} "
          f"(bars {h.BAR_FACTOR[t][0]:.4f} {h.BAR_FACTOR[t][1]:.4f})")
    assert norm <= h.BAR_FACTOR[t][0] and comp <= h.BAR_FACTOR[t][1]


FACTOR_CASES = [(name, t, n, nb) for t in "sdcz" for (n, nb) in h.sizes_of(t) for name in h.FAMILIES]


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("name,t,n,nb", FACTOR_CASES)
def test_factor_accuracy(dlaf, grid, name, t, n, nb, uplo):
    check_factor(dlaf, grid, name, t, n, nb, uplo)


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("n,nb", [(129, 64), (515, 128)])
@pytest.mark.parametrize("t", "dz")
def test_factor_accuracy_every_schedule(dlaf, grid, schedule, t, n, nb, uplo):
    check_factor(dlaf, grid, "geo", t, n, nb, uplo, schedule)


# ------------------------------------------------------------------------------------------- accuracy of the solves
@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("nrhs", h.NRHS)
@pytest.mark.parametrize("n,nb", h.SOLVE_SIZES)
@pytest.mark.parametrize("name", h.SOLVE_FAMILIES)
@pytest.mark.parametrize("t", "dz")
def test_solve_accuracy(dlaf, grid, t, name, n, nb, nrhs, uplo):
    """a backward measure only: at a condition number of 1e10 a forward error means nothing"""
    a0, b0 = h.family(name, t, n), h.rhs(t, n, nrhs)
    # cholesky_factorization, then p?potrs
    abuf, a = h.padded(a0)
    assert dlaf.cholesky_factorization(grid, uplo, a, nb) == 0
    fac0 = abuf.copy()
    bbuf, b = h.padded(b0)
    assert dlaf.pxpotrs(uplo, n, nrhs, a, 1, 1, desc_of(grid, n, n, nb, n + h.PAD), b, 1, 1,
                        desc_of(grid, n, nrhs, nb, n + h.PAD)) == 0
    assert h.same_bits(abuf, fac0) and (bbuf[n:, :] == h.SENTINEL).all()
    r1 = h.solve_ratio(t, a0, b0, b)
    # DeviceMatrix.factorize, then potrs_device
    m = dlaf.DeviceMatrix(grid, h.DT[t], uplo, n, nb)
    m.upload(np.asfortranarray(a0))
    assert m.factorize() == 0
    g = dlaf.GeneralDeviceMatrix(grid, h.DT[t], n, nrhs, nb)
    g.upload(np.asfortranarray(b0))
    dlaf.potrs_device(uplo, m, g)
    x = np.zeros((n, nrhs), h.DT[t], order="F")
    g.download(x)
    r2 = h.solve_ratio(t, a0, b0, x)
    print(f"RATIO solve {t} {name} n={n} nb={nb} nrhs={nrhs} {uplo}: p?potrs {r1:.4f} potrs_device {r2:.4f} "
          f"(bar {h.BAR_SOLVE[t]:.4f})")
    assert r1 <= h.BAR_SOLVE[t] and r2 <= h.BAR_SOLVE[t]


# --------------------------------------------------------------------------------------- exact scale equivariance
@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("which", ["random_hpd", "geo"])
@pytest.mark.parametrize("t", "sdcz")
def test_scaling_by_a_power_of_four_is_exact(dlaf, grid, oracle, t, which, uplo):
    """The factor of 4^k A is 2^k x the factor of A bit for bit: the scaling commutes with every rounding, square root
    and inversion, and the summation order is fixed; a difference means an absolute threshold hides somewhere."""
    n, nb = 515, 128
    a0 = oracle.set_random_hpd(n, nb, h.DT[t]) if which == "random_hpd" else h.family("geo", t, n)
    base = np.array(a0, order="F")
    assert dlaf.cholesky_factorization(grid, uplo, base, nb) == 0
    k = h.scale_exponent(t)
    for e in (k, -k):
        got = h.scaled(a0, e)
        assert dlaf.cholesky_factorization(grid, uplo, got, nb) == 0
        assert np.isfinite(h.lower_of(got, uplo)).all()
        assert h.tri_same_bits(got, h.times_pow2(base, e), uplo), (t, which, uplo, e)


# ------------------------------------------------------------------------------------------ not positive definite
PLANTED_600 = [(0,), (63,), (64,), (255,), (256,), (511,), (512,), (599,), (300, 101)]
FULL = [("planted", 515, 128, (514,))] + [("planted", 600, 256, w) for w in PLANTED_600] + \
       [("through", 600, 256, w) for w in ("tile0", "tile1", "last")]
SUBSET = [("planted", 600, 256, (0,)), ("planted", 600, 256, (256,)), ("planted", 600, 256, (599,)),
          ("through", 600, 256, "tile1")]
SINGLE = [("planted", 600, 256, (256,)), ("planted", 600, 256, (599,))]
NONFINITE = [("nan", 600, 256, (j, j)) for j in h.NONFINITE_DIAG] + [("nan", 600, 256, ij) for ij in h.NONFINITE_OFF] + \
            [("inf", 600, 256, ij) for ij in h.NONFINITE_OFF]


@functools.lru_cache(maxsize=None)
def not_spd(t, kind, n, where):
    """(matrix, the info the textbook algorithm gives)"""
    if kind == "planted":
        a = h.planted(t, n, where)
    elif kind == "through":
        a = np.array(h.through_updates(t, where), order="F")
    else:
        a = h.with_value(h.family("one_small", t, n), where[0], where[1], np.nan if kind == "nan" else np.inf)
    info = h.unblocked_info(a)
    if kind == "planted":
        assert info == min(where) + 1
    elif kind in ("nan", "inf"):
        assert info == where[0] + 1
    else:
        lo, hi = h.THROUGH_RANGE[where]
        assert lo < info <= hi
    return h.frozen(a), info


def fresh_factor(dlaf, grid, t, uplo, n, nb, spd):
    m = dlaf.DeviceMatrix(grid, h.DT[t], uplo, n, nb)
    m.upload(spd)
    assert m.factorize() == 0 and m.local_info() == 0
    out = np.full((n, n), h.SENTINEL, h.DT[t], order="F")
    m.download(out)
    return out


def check_not_spd(dlaf, grid, t, kind, n, nb, where, uplo):
    a0, expect = not_spd(t, kind, n, where)
    # the host entries: exactly the textbook info; nothing outside the triangle moves
    buf, a = h.padded(a0)
    buf0 = buf.copy()
    got = dlaf.cholesky_factorization(grid, uplo, a, nb)
    print(f"INFO {t} {kind} n={n} nb={nb} {where} {uplo}: {got} (expected {expect})")
    assert got == expect
    assert h.untouched(buf, buf0, uplo)
    buf, a = h.padded(a0)
    assert dlaf.pxpotrf(uplo, n, a, 1, 1, desc_of(grid, n, n, nb, n + h.PAD)) == expect
    assert h.untouched(buf, buf0, uplo)
    # the resident handle: the same info, and nothing of the aborted run survives into the next one
    m = dlaf.DeviceMatrix(grid, h.DT[t], uplo, n, nb)
    m.upload(np.asfortranarray(a0))
    assert m.factorize() == expect
    assert m.local_info() == expect
    spd = np.asfortranarray(h.family("geo", t, n))
    m.upload(spd)
    assert m.factorize() == 0 and m.local_info() == 0
    again = np.full((n, n), h.SENTINEL, h.DT[t], order="F")
    m.download(again)
    assert h.tri_same_bits(again, fresh_factor(dlaf, grid, t, uplo, n, nb, spd), uplo)
    assert np.isfinite(again[h.tri_mask(n, uplo)]).all()


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("kind,n,nb,where", FULL)
@pytest.mark.parametrize("t", "dz")
def test_not_positive_definite(dlaf, grid, t, kind, n, nb, where, uplo):
    check_not_spd(dlaf, grid, t, kind, n, nb, where, uplo)


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("kind,n,nb,where", SINGLE)
@pytest.mark.parametrize("t", "sc")
def test_not_positive_definite_single_precision(dlaf, grid, t, kind, n, nb, where, uplo):
    check_not_spd(dlaf, grid, t, kind, n, nb, where, uplo)


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("kind,n,nb,where", SUBSET)
@pytest.mark.parametrize("t", "dz")
def test_not_positive_definite_every_schedule(dlaf, grid, schedule, t, kind, n, nb, where, uplo):
    check_not_spd(dlaf, grid, t, kind, n, nb, where, uplo)


@pytest.mark.parametrize("uplo", "LU")
@pytest.mark.parametrize("kind,n,nb,where", NONFINITE)
@pytest.mark.parametrize("t", "dz")
def test_nan_and_inf(dlaf, grid, t, kind, n, nb, where, uplo):
    """NaN on the diagonal fails there; NaN or +Inf at (i, j) below it poisons row i of the factor only, so pivot i is the
    first to become NaN (-Inf).  The upper variant carries the same value at (j, i)."""
    check_not_spd(dlaf, grid, t, kind, n, nb, where, uplo)


CHAIN_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import dla_future_amd as d
import hard_spd as h
d.initialize()
g = d.Grid.single()
for t in "dz":
    for kind, n, nb, where in %r:
        a0 = h.planted(t, n, where) if kind == "planted" else np.array(h.through_updates(t, where), order="F")
        for uplo in "LU":
            a = np.array(a0, order="F")
            info = d.cholesky_factorization(g, uplo, a, nb)
            m = d.DeviceMatrix(g, h.DT[t], uplo, n, nb)
            m.upload(a0)
            print("INFO", t, kind, where, uplo, info, m.factorize(), flush=True)
"""


def test_not_positive_definite_chain_potrf():
    """the chain form of the tile POTRF: DLAF_MI355X_POTRF is read once per process, so one child runs the subset"""
    code = CHAIN_CHILD % (ROOT, os.path.join(ROOT, "tests"), SUBSET)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, DLAF_MI355X_POTRF="chain"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("INFO")]
    print("\n".join(lines))
    want = [f"INFO {t} {kind} {where} {uplo} {not_spd(t, kind, n, where)[1]} {not_spd(t, kind, n, where)[1]}"
            for t in "dz" for kind, n, nb, where in SUBSET for uplo in "LU"]
    assert lines == want


# --------------------------------------------------------------------------------------- the generalized drivers
def random_hermitian(n, dt, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n)).astype(dt)
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.uniform(-1, 1, (n, n)).astype(dt)
    return np.asfortranarray((a + a.conj().T).astype(dt))


@pytest.mark.parametrize("j", [0, 200])
@pytest.mark.parametrize("t", "dz")
def test_generalized_drivers_refuse_an_indefinite_b(dlaf, grid, t, j):
    """a B that is not positive definite: both drivers raise with the info of its factorization and leave every array
    of the caller as it was; an ordinary call afterwards is held to the bars of test_hermitian_generalized_eigensolver"""
    from oracle import tridiag as td
    n, nb = 300, 64
    dt = h.DT[t]
    a0 = random_hermitian(n, dt, 21 + n)
    b0 = random_hermitian(n, dt, 22 + n)
    b0 = np.asfortranarray(b0 @ b0.conj().T / n + np.eye(n, dtype=dt) * 2)
    bad = b0.copy(order="F")
    bad[j, j] = -abs(bad[j, j])
    assert h.unblocked_info(bad) == j + 1 and h.decisive(bad)
    rdt = np.zeros(1, dt).real.dtype
    for values_only in (False, True):
        (abuf, a), (bbuf, b) = h.padded(a0), h.padded(bad)
        zbuf, z = h.padded(np.full((n, n), 3.3, dt))
        w = np.full(n, 5.5, rdt)
        keep = [x.copy() for x in (abuf, bbuf, zbuf, w)]
        with pytest.raises(RuntimeError, match=rf"returned {j + 1}$"):
            if values_only:
                dlaf.hermitian_generalized_eigenvalues(grid, "L", a, b, nb, w=w)
            else:
                dlaf.hermitian_generalized_eigensolver(grid, "L", a, b, nb, z=z)
        for x, x0 in zip((abuf, bbuf, zbuf, w), keep):
            assert h.same_bits(x, x0)
    # an ordinary call afterwards
    err = td.error_of(dt)
    w, z = dlaf.hermitian_generalized_eigensolver(grid, "L", a0.copy(order="F"), b0.copy(order="F"), nb)
    assert np.all(np.diff(w) >= 0)
    gram = z.conj().T @ b0 @ z
    assert np.abs(gram - np.eye(n)).max() <= 10 * n * err * np.abs(b0).max()
    res = a0 @ z - (b0 @ z) * w[None, :]
    assert np.abs(res).max() <= 10 * n * err * max(1.0, np.abs(a0).max() * np.abs(w).max())
    w2 = dlaf.hermitian_generalized_eigenvalues(grid, "L", a0.copy(order="F"), b0.copy(order="F"), nb)
    assert np.abs(w2 - w).max() <= 10 * n * err * max(1.0, np.abs(w).max())
