"""GPU tests of tridiagonal_eigensolver (the divide & conquer solver of kernels_tridiag_dc.hip) against the
extended-precision reference of oracle/tridiag.py (Sturm-count bisection in long double on the exact inputs), with every
bar relative to |T|_2: the xSTEDC test-matrix families at leaf, merge and tree-level edges, exact scale equivariance
under powers of two, non-power-of-two scales, other leaf sizes, many tree levels, and the eigensolver drivers on scaled
matrices.

The bars are those of test_gpu_eigensolver.py with their absolute floor max(1, .) removed: eigenvalues n error |T|,
residual max_j |T z_j - w_j z_j|_inf <= 2 n error |T|, orthogonality max |Z^T Z - I| <= 10 n error, where
error = 2 eps is the reference's TypeUtilities<T>::error.  Every check prints its ratios to the bars (RATIO lines).

Cost: the whole file, CPU references included (about two thirds of it), runs in under a minute next to one MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sl

from oracle import tridiag as td

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
NB = 64  # the solver's tree is cut by its leaf size, not by nb
SMALL = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)
# the families also run at n = 1000 (several tree levels): the reference costs ~2.5 s per matrix there
LARGE = {"d": ("glued_wilk_1e-14", "dlatms_b", "graded"), "s": ("rand_mixed", "dlatms_c")}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@functools.lru_cache(maxsize=None)
def case(family, n, t):
    """(d, e, reference eigenvalues in long double): one reference per input, shared by the tests below"""
    d, e = td.tridiag_family(family, n, DT[t])
    d.flags.writeable = False
    e.flags.writeable = False
    return d, e, td.sturm_eigvals(d, e)


def check(what, d, e, w, z, t, ref, eig=True):
    n = len(d)
    f = td.check_tridiag_solution(d, e, w, z, DT[t], w_ref=ref)
    u = td.error_of(DT[t]) / np.finfo(DT[t]).eps  # check_tridiag_solution reports in units of eps
    ratios = {"eig": f["eig"] / (n * u) if eig else 0.0, "residual": f["residual"] / (2 * n * u),
              "orth": f["orth"] / (10 * n * u)}
    print(f"RATIO {what} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
    assert f["sorted"], (what, f)
    assert all(v <= 1 for v in ratios.values()), (what, ratios, f)  # each on its own: a NaN finding fails
    return f


def solve(dlaf, d, e):
    w, z = dlaf.tridiagonal_eigensolver(np.array(d), np.array(e), NB)
    assert w.dtype == d.dtype and z.shape == (len(d), len(d))
    return w, z


def exact_checks(family, d, w):
    """the families whose answer is exact in floating point"""
    if family == "zero":
        assert not w.any(), w
    elif family == "const":
        assert np.all(w == d[0]), w
    elif family == "diag":
        assert np.array_equal(w, np.sort(d)), w


# ---------------------------------------------------------------------------------------------------- families
@pytest.mark.parametrize("t", ["d", "s"])
@pytest.mark.parametrize("family", td.FAMILIES)
def test_families(dlaf, family, t):
    for n in SMALL + ((1000,) if family in LARGE[t] else ()):
        d, e, ref = case(family, n, t)
        w, z = solve(dlaf, d, e)
        exact_checks(family, d, w)
        check(f"{t} {family} n={n}", d, e, w, z, t, ref)


# ------------------------------------------------------------------------------------ exact scale equivariance
EQUI_K = {"d": (-600, -40, -1, 1, 40, 600), "s": (-60, -20, -1, 1, 20, 60)}


def equivariance_input(family, n, t):
    """unscaled input with every entry >= 2^-30 in magnitude or exactly zero: no 2^k T below is subnormal"""
    d, e = (x.copy() for x in td.tridiag_family(family, n, DT[t], seed=5))
    d[np.abs(d) < 2.0 ** -30] = 0
    e[np.abs(e) < 2.0 ** -30] = 0
    return d, e


@pytest.mark.parametrize("t", ["d", "s"])
@pytest.mark.parametrize("family", ["rand_mixed", "glued_wilk_sqrteps", "dlatms_b"])
@pytest.mark.parametrize("n", [200, 1000])
def test_scale_equivariance_is_exact(dlaf, family, n, t):
    """w(2^k T) == 2^k w(T) and z(2^k T) == z(T) bit for bit: the solver normalises T by a power of two, so every
    deflation decision, root and rotation is the same.  First: two runs of one input agree bit for bit."""
    d, e = equivariance_input(family, n, t)
    w, z = solve(dlaf, d, e)
    w2, z2 = solve(dlaf, d, e)
    assert np.array_equal(w, w2) and np.array_equal(z, z2), (family, n, t, "two runs of one input differ")
    bad = []
    for k in EQUI_K[t]:
        wk, zk = solve(dlaf, np.ldexp(d, k), np.ldexp(e, k))
        if not (np.array_equal(wk, np.ldexp(w, k)) and np.array_equal(zk, z)):
            bad.append((k, float(np.abs(np.ldexp(wk, -k) - w).max() / np.abs(w).max()), float(np.abs(zk - z).max())))
    assert not bad, (family, n, t, "(k, max|2^-k w_k - w| / |T|, max|z_k - z|):", bad)


# ------------------------------------------------------------------------------------ non-power-of-two scales
ALPHAS = {"d": (1e-12, 1e-6, 1e6, 1e12), "s": (1e-5, 1e5)}
SCALED = {"d": [("rand_mixed", 200), ("dlatms_b", 200), ("glued_wilk_1e-14", 200), ("rand_neg", 1000)],
          "s": [("rand_mixed", 200), ("dlatms_b", 200), ("glued_wilk_sqrteps", 200), ("rand_alt", 1000)]}


@pytest.mark.parametrize("t", ["d", "s"])
def test_scaled(dlaf, t):
    for family, n in SCALED[t]:
        d0, e0 = td.tridiag_family(family, n, DT[t])
        for alpha in ALPHAS[t]:
            # the reference is computed on the scaled input as the solver sees it (rounded to the type)
            d, e = d0 * DT[t](alpha), e0 * DT[t](alpha)
            w, z = solve(dlaf, d, e)
            check(f"{t} {family} n={n} alpha={alpha:g}", d, e, w, z, t, td.sturm_eigvals(d, e))


# ------------------------------------------------------------------------------------------------- leaf sizes
LEAF_CASES = [("rand_mixed", 200), ("glued_wilk_1e-14", 129), ("rho0", 200), ("zero_e_inside", 128), ("repeated", 200),
              ("graded", 65), ("wilkinson", 63), ("dlatms_a", 127), ("diag", 64), ("clement", 3), ("rand_alt", 1),
              ("rand_neg", 2)]
LEAF_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import dla_future_amd as dl
from oracle import tridiag as td
dl.initialize()
out = {}
for t, dt in (("d", np.float64), ("s", np.float32)):
    for i, (family, n) in enumerate(%r):
        d, e = td.tridiag_family(family, n, dt)
        out[f"{t}{i}_w"], out[f"{t}{i}_z"] = dl.tridiagonal_eigensolver(d, e, 64)
np.savez(%r, **out)
print("DONE", flush=True)
"""


@pytest.mark.fresh_parent
def test_leaf_sizes(tmp_path):
    """DLAF_MI355X_DC_LEAF in {1, 2, 3, 17, 64}, read once per process: one child per size, one after the other.
    One-row leaves (two Cuppen corrections on one diagonal entry), leaves of two and three rows, odd leaves, the
    default."""
    for leaf in (1, 2, 3, 17, 64):
        path = str(tmp_path / f"leaf{leaf}.npz")
        r = subprocess.run([sys.executable, "-c", LEAF_CHILD % (ROOT, LEAF_CASES, path)], cwd=ROOT,
                           env=dict(os.environ, DLAF_MI355X_DC_LEAF=str(leaf)), capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, (leaf, r.stdout[-2000:], r.stderr[-3000:])
        res = np.load(path)
        for t in ("d", "s"):
            for i, (family, n) in enumerate(LEAF_CASES):
                d, e, ref = case(family, n, t)
                w, z = res[f"{t}{i}_w"], res[f"{t}{i}_z"]
                exact_checks(family, d, w)
                check(f"leaf={leaf} {t} {family} n={n}", d, e, w, z, t, ref)


# ------------------------------------------------------------------------------------------------ many levels
@pytest.mark.parametrize("t,n", [("d", 4097), ("s", 2049)])
@pytest.mark.parametrize("family", ["rand_mixed", "dlatms_b"])
def test_many_levels(dlaf, family, t, n):
    """seven and six levels of merges above the leaves (one of them a lone leaf): residual and orthogonality, |T| from
    LAPACK"""
    d, e = td.tridiag_family(family, n, DT[t])
    w, z = solve(dlaf, d, e)
    ref = sl.eigvalsh_tridiagonal(d.astype(np.float64), e.astype(np.float64), lapack_driver="stev")
    check(f"{t} {family} n={n}", d, e, w, z, t, ref, eig=False)


# ------------------------------------------------------------------------------------------- drivers at scale
def random_hermitian(n, dt, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, n)).astype(dt)
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.uniform(-1, 1, (n, n)).astype(dt)
    return np.asfortranarray((a + a.conj().T).astype(dt))


@pytest.mark.parametrize("t,n,nb,alphas", [("d", 300, 64, (2.0 ** -40, 1e-12, 2.0 ** 40)),
                                           ("z", 300, 64, (2.0 ** -40, 1e-12, 2.0 ** 40)),
                                           ("d", 1100, 256, (2.0 ** -40, 1e-12, 2.0 ** 40)),
                                           ("z", 1100, 256, (2.0 ** -40, 1e-12, 2.0 ** 40)),
                                           ("s", 300, 64, (2.0 ** -20, 1e-5, 2.0 ** 20)),
                                           ("c", 300, 64, (2.0 ** -20, 1e-5, 2.0 ** 20))])
def test_hermitian_eigensolver_scaled(dlaf, t, n, nb, alphas):
    """hermitian_eigensolver(alpha A): every stage keeps its accuracy relative to |alpha A|"""
    dt = DT[t]
    wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    err = td.error_of(dt)
    grid = dlaf.Grid.single()
    a1 = random_hermitian(n, dt, 31 + n)
    for alpha in alphas:
        a0 = np.asfortranarray(a1 * np.dtype(dt).type(alpha))
        w, z = dlaf.hermitian_eigensolver(grid, "L", a0.copy(order="F"), nb)
        aw, zw = a0.astype(wide), z.astype(wide)
        ref = np.linalg.eigvalsh(aw)
        norm = float(np.abs(ref).max())
        ratios = {"eig": float(np.abs(w - ref).max()) / (n * err * norm),
                  "residual": float(np.abs(aw @ zw - zw * w[None, :]).max()) / (2 * n * err * norm),
                  "orth": float(np.abs(zw.conj().T @ zw - np.eye(n)).max()) / (10 * n * err)}
        print(f"RATIO driver {t} n={n} nb={nb} alpha={alpha:g} " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))
        assert np.all(np.diff(w) >= 0), (t, n, alpha)
        assert all(v <= 1 for v in ratios.values()), (t, n, nb, alpha, ratios)


@pytest.mark.parametrize("t", ["d", "z"])
def test_hermitian_generalized_eigensolver_scaled(dlaf, t):
    """hermitian_generalized_eigensolver(alpha A, beta B) with powers of two: (sqrt(beta) Z, (beta / alpha) w) solves
    the unscaled problem exactly as well and is held to the bars of test_hermitian_generalized_eigensolver"""
    dt = DT[t]
    err = td.error_of(dt)
    n, nb = 300, 64
    grid = dlaf.Grid.single()
    a0 = random_hermitian(n, dt, 21 + n)
    b0 = random_hermitian(n, dt, 22 + n)
    b0 = np.asfortranarray(b0 @ b0.conj().T / n + np.eye(n, dtype=dt) * 2)
    for la, lb in ((-30, 20), (30, -20)):
        alpha, beta = 2.0 ** la, 2.0 ** lb
        ws, zs = dlaf.hermitian_generalized_eigensolver(grid, "L", np.asfortranarray(a0 * alpha),
                                                        np.asfortranarray(b0 * beta), nb)
        z, w = zs * np.sqrt(beta), ws * (beta / alpha)
        assert np.all(np.diff(w) >= 0)
        orth = np.abs(z.conj().T @ b0 @ z - np.eye(n)).max()
        res = np.abs(a0 @ z - (b0 @ z) * w[None, :]).max()
        obar = 10 * n * err * np.abs(b0).max()
        rbar = 10 * n * err * max(1.0, np.abs(a0).max() * np.abs(w).max())
        print(f"RATIO gen {t} alpha=2^{la} beta=2^{lb} orth={orth / obar:.3g} residual={res / rbar:.3g}")
        assert orth <= obar, (t, la, lb, orth, obar)
        assert res <= rbar, (t, la, lb, res, rbar)
