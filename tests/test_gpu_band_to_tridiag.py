"""band_to_tridiagonal and its back-transformation on every kernel path, against the long-double checkers of
oracle/tridiag.py (backward error on probe columns, unitarity of every reflector, layout of v, spectrum).

launch_band_to_tridiag (kernels_tridiag.hip) picks one of three kernels:
  * b2t_reg_kernel<EARLY = true>:  s, d, c at band 128 (loads of a step issued before the wait for the predecessor);
  * b2t_reg_kernel<EARLY = false>: s, d, c at band < 128;
  * b2t_kernel (generic):          z at every band, every type at band 129 .. 256, and s, d, c under
                                   DLAF_MI355X_B2T_KERNEL=generic (configuration children below).
bt_band_to_tridiagonal runs the fused kernel for d at band 128 (kernels_bt.hip) and the batched products otherwise.

Sweeps in flight: a launch holds min(256, (n / b + 2) / 2 + 1) workgroups, so many concurrent hand-offs only happen at
small bands or at n >= 12 b.  Scale: the device xLARFG sums squares unscaled, so the band is normalised by a power of
two first; the equivariance cases hold the stage to that bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (type, band, nb) of each path.  nb only changes the tile layout the band is extracted from.
REG_EARLY = [(t, 128, 128) for t in "sdc"]
REG = [(t, b, 2 * b if b < 64 else b) for t in "sdc" for b in (2, 3, 64, 127)]
GENERIC = [("z", b, b) for b in (2, 16, 128)] + [(t, b, nb) for t in "sdcz" for b in (129, 192, 255, 256)
                                                  for nb in (b, 2 * b)]
PATHS = REG_EARLY + REG + GENERIC


def path_id(p):
    return f"{p[0]}-b{p[1]}-nb{p[2]}"


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


@pytest.fixture(scope="module")
def td():
    from oracle import tridiag
    return tridiag


def random_band(n, band, dt, seed, quantum=None):
    """Hermitian, lower band of width `band`, entries uniform in [-1, 1] (multiples of `quantum` when given)."""
    rng = np.random.default_rng(seed)
    re = rng.uniform(-1, 1, (n, n))
    im = rng.uniform(-1, 1, (n, n)) if np.dtype(dt).kind == "c" else None
    if quantum is not None:
        re = np.round(re / quantum) * quantum
        im = None if im is None else np.round(im / quantum) * quantum
    a = re.astype(dt)
    if im is not None:
        a = a + 1j * im.astype(dt)
    a = np.tril(a)
    a = a + np.tril(a, -1).conj().T
    if np.dtype(dt).kind == "c":
        a[np.arange(n), np.arange(n)] = a.diagonal().real
    i, j = np.indices((n, n))
    a[np.abs(i - j) > band] = 0
    return np.asfortranarray(a.astype(dt))


def b2t(dlaf, grid, a0, nb, band):
    """band_to_tridiagonal on a0 with junk outside its lower band (the reflectors of reduction_to_band below it, the
    upper triangle above): the host array must come back bit-identical."""
    n = a0.shape[0]
    a = a0.copy(order="F")
    i, j = np.indices((n, n))
    a[i - j > band] = 7.7
    a[j > i] = -9.9
    before = a.copy(order="F")
    d, e, v = dlaf.band_to_tridiagonal(grid, a, nb, band)
    assert np.array_equal(a, before)
    assert d.shape == (n,) and e.shape == (max(n - 1, 0),) and v.shape == (n, n)
    return d, e, v


def check(td, a0, band, d, e, v, what):
    checks = td.b2t_checks(a0, band, d, e, v)
    bad = td.b2t_failures(checks)
    assert not bad, (what, bad)
    return checks


def edge_sizes(b):
    return sorted({n for n in (2, 3, b - 1, b + 1, b + 2, 2 * b - 1, 2 * b, 2 * b + 1, 3 * b + 2) if n >= 1})


def in_flight_size(b):
    """the smallest n at which a launch holds >= 8 workgroups"""
    return 12 * b + 3


# ------------------------------------------------------------------------------------------ paths x edges
@pytest.mark.parametrize("path", PATHS, ids=path_id)
def test_b2t_paths_at_edges(dlaf, grid, td, path):
    t, band, nb = path
    sizes = edge_sizes(band)
    # the >= 8 sweeps in flight case once per (type, band), and at bands above 128 for the smallest and largest band
    if nb == band or band < 129:
        if band < 129 or band in (129, 256):
            sizes.append(in_flight_size(band))
    for n in sizes:
        a0 = random_band(n, band, DT[t], 1000 + n + band)
        d, e, v = b2t(dlaf, grid, a0, nb, band)
        check(td, a0, band, d, e, v, (t, n, nb, band))


@pytest.mark.parametrize("t,n,band", [("d", 1000, 4), ("c", 900, 3), ("s", 700, 2), ("z", 1100, 8)])
def test_b2t_many_sweeps_in_flight(dlaf, grid, td, t, n, band):
    """70 - 180 workgroups chase bulges at once"""
    a0 = random_band(n, band, DT[t], 7 + n)
    d, e, v = b2t(dlaf, grid, a0, 4 * band, band)
    check(td, a0, band, d, e, v, (t, n, band))


# ------------------------------------------------------------------------------------------ structured bands
@pytest.mark.parametrize("t,n,band", [("c", 200, 8), ("c", 300, 128), ("z", 200, 8), ("z", 300, 192)])
def test_b2t_complex_corner(dlaf, grid, td, t, n, band):
    """A complex band that is already tridiagonal, with complex subdiagonal entries: every reflector comes from
    ss == 0, Im alpha != 0 (a 1 x 1 reflector that only rotates the phase).  And a complex band with real entries."""
    rng = np.random.default_rng(n + band)
    dt = DT[t]
    a0 = np.zeros((n, n), dtype=dt, order="F")
    a0[np.arange(n), np.arange(n)] = rng.uniform(-1, 1, n)
    sub = rng.uniform(-1, 1, n - 1) + 1j * rng.uniform(-1, 1, n - 1)
    a0[np.arange(1, n), np.arange(n - 1)] = sub
    a0[np.arange(n - 1), np.arange(1, n)] = sub.conj()
    d, e, v = b2t(dlaf, grid, a0, band, band)
    check(td, a0, band, d, e, v, (t, n, band, "tridiagonal"))
    # |e| of a tridiagonal Hermitian matrix is the modulus of its subdiagonal
    assert np.allclose(np.abs(e), np.abs(np.diagonal(a0, -1)), rtol=4 * td.error_of(dt), atol=0), (t, n, band)
    a1 = random_band(n, band, np.float64, 3 + n).astype(dt)
    d, e, v = b2t(dlaf, grid, a1, band, band)
    check(td, a1, band, d, e, v, (t, n, band, "real entries"))


ZERO_DIAG_PATHS = [("d", 128), ("s", 128), ("c", 128), ("s", 16), ("d", 3), ("c", 64), ("z", 16), ("d", 192), ("z", 256)]


@pytest.mark.parametrize("t,band", ZERO_DIAG_PATHS)
def test_b2t_zero_and_diagonal_bands(dlaf, grid, td, t, band):
    """No NaN, every tau 0 (v all zero), d the diagonal bit for bit, e zero."""
    n = 300
    dt = DT[t]
    rng = np.random.default_rng(band)
    for diag in (np.zeros(n), rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 30, n)):
        a0 = np.asfortranarray(np.diag(diag).astype(dt))
        d, e, v = b2t(dlaf, grid, a0, band, band)
        assert np.array_equal(d, diag.astype(d.dtype)), (t, band)
        assert not np.any(e) and not np.any(v), (t, band)
        check(td, a0, band, d, e, v, (t, band))


# ------------------------------------------------------------------------------------------ scale
EQUI_PATHS = [("s", 16), ("s", 128), ("c", 128), ("d", 16), ("s", 192), ("d", 192), ("c", 8), ("z", 16)]
EQUI_J = {np.float32: [30, -30, 64, -64, 70, -70, -100, 120], np.float64: [200, -200, 520, -520, 600, -600, 1000, -1000]}


@pytest.mark.parametrize("t,band", EQUI_PATHS)
def test_b2t_power_of_two_equivariance(dlaf, grid, td, t, band):
    """Entries >= 2^-20 in magnitude or zero, so 2^j A is exact: b2t(2^j A) must return 2^j (d, e) and the same v, bit
    for bit, over the whole exponent range of the type."""
    n = 2 * band + 37
    dt = DT[t]
    rt = np.zeros(0, dtype=dt).real.dtype.type
    a0 = random_band(n, band, dt, 17 + band, quantum=2.0 ** -20)
    d0, e0, v0 = b2t(dlaf, grid, a0, band, band)
    check(td, a0, band, d0, e0, v0, (t, band, 0))
    for j in EQUI_J[rt]:
        aj = np.asfortranarray(a0 * rt(2.0) ** j)
        assert np.array_equal(np.ldexp(aj.real, -j), a0.real)
        d, e, v = b2t(dlaf, grid, aj, band, band)
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(e)) and np.all(np.isfinite(v)), (t, band, j)
        assert np.array_equal(v, v0), (t, band, j, int(np.sum(v != v0)))
        assert np.array_equal(d, np.ldexp(d0, j)) and np.array_equal(e, np.ldexp(e0, j)), (t, band, j)


SCALE_PATHS = [("s", 16), ("s", 128), ("c", 64), ("s", 200), ("d", 16), ("d", 128), ("z", 32), ("d", 256)]


@pytest.mark.parametrize("t,band", SCALE_PATHS)
def test_b2t_extreme_scale(dlaf, grid, td, t, band):
    """A scaled by 10^(+-20) (fp32) / 10^(+-200) (fp64), not powers of two: held to the checkers' own bars"""
    n = 2 * band + 41
    dt = DT[t]
    p = 20 if np.zeros(0, dtype=dt).real.dtype == np.float32 else 200
    a0 = random_band(n, band, np.complex128 if np.dtype(dt).kind == "c" else np.float64, 23 + band)
    for alpha in (10.0 ** p, 10.0 ** -p):
        a = np.asfortranarray((a0 * alpha).astype(dt))
        d, e, v = b2t(dlaf, grid, a, band, band)
        check(td, a, band, d, e, v, (t, band, alpha))


@pytest.mark.parametrize("t,band", [("s", 8), ("d", 8), ("c", 128), ("z", 16), ("d", 192)])
def test_b2t_graded(dlaf, grid, td, t, band):
    """D B D with D = diag(2^(-i s)): the entries span 2^-56 (fp32) / 2^-480 (fp64) from the first row to the last,
    which keeps every sum of squares of the normalised band normal"""
    n = 200
    dt = DT[t]
    span = 56 if np.zeros(0, dtype=dt).real.dtype == np.float32 else 480
    s = span / 2 / (n - 1)
    dg = 2.0 ** (-np.arange(n) * s)
    b0 = random_band(n, band, np.complex128 if np.dtype(dt).kind == "c" else np.float64, 31 + band)
    a = np.asfortranarray((dg[:, None] * b0 * dg[None, :]).astype(dt))
    d, e, v = b2t(dlaf, grid, a, band, band)
    check(td, a, band, d, e, v, (t, band))


# ------------------------------------------------------------------------------------------ back-transformation
BT_K = (1, 15, 64, 65, 300)


@pytest.mark.parametrize("path", [p for p in PATHS if p[2] == p[1] or p[1] < 129], ids=path_id)
def test_bt_b2t_paths(dlaf, grid, td, path):
    """bt_band_to_tridiagonal from the v of every b2t path, E a padded-ld view whose sentinel rows above and below and the
    column next to it stay bit-identical, v unchanged.  Reference: apply_q in long double, bar 20 n error."""
    t, band, nb = path
    dt = DT[t]
    n = 2 * band + 1 if band >= 64 else 150
    a0 = random_band(n, band, dt, 41 + n)
    d, e, v = b2t(dlaf, grid, a0, nb, band)
    rng = np.random.default_rng(n + band)
    kmax = max(BT_K)
    e0 = rng.uniform(-1, 1, (n, kmax))
    if np.dtype(dt).kind == "c":
        e0 = e0 + 1j * rng.uniform(-1, 1, (n, kmax))
    e0 = e0.astype(dt)
    ldt = np.clongdouble if np.dtype(dt).kind == "c" else np.longdouble
    ref = td.apply_q(v.astype(ldt), band, e0.astype(ldt))
    tol = 20 * n * td.error_of(dt)
    for k in BT_K:
        store = np.full((n + 7, k + 1), -3.25, dtype=dt, order="F")
        emat = store[3:n + 3, :k]
        emat[...] = e0[:, :k]
        sentinel = store.copy(order="F")
        v_in = v.copy(order="F")
        dlaf.bt_band_to_tridiagonal(band, emat, v_in)
        assert np.array_equal(v_in, v), (t, band, k)
        assert np.array_equal(store[:3], sentinel[:3]) and np.array_equal(store[n + 3:], sentinel[n + 3:]), (t, band, k)
        assert np.array_equal(store[:, k:], sentinel[:, k:]), (t, band, k)
        err = float(np.abs(emat - ref[:, :k]).max())
        assert err <= tol, (t, n, band, k, err, tol)


# ------------------------------------------------------------------------------------------ configuration children
CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import dla_future_amd as d
from test_gpu_band_to_tridiag import random_band, DT
d.initialize()
g = d.Grid.single()
out = {}
for t, n, band, seed in %(cases)r:
    a0 = random_band(n, band, DT[t], seed)
    dd, ee, v = d.band_to_tridiagonal(g, a0.copy(order="F"), band * max(1, 128 // band), band)
    key = "%%s_%%d_%%d" %% (t, n, band)
    out[key + "_d"], out[key + "_e"] = dd, ee
    if n <= %(keep_v)d:
        out[key + "_v"] = v
    else:
        out[key + "_vhash"] = np.array([hashlib.sha1(v[:, c].tobytes()).hexdigest() for c in range(n)])
    for k in %(bt_k)r:
        rng = np.random.default_rng(n + k)
        e0 = rng.uniform(-1, 1, (n, k))
        if np.dtype(DT[t]).kind == "c":
            e0 = e0 + 1j * rng.uniform(-1, 1, (n, k))
        em = np.asfortranarray(e0.astype(DT[t]))
        d.bt_band_to_tridiagonal(band, em, v)
        out[key + "_bt%%d" %% k] = em
np.savez(%(path)r, **out)
print("CHILD DONE", flush=True)
"""

# the hand-off cases: d 4096/128 (EARLY register kernel, 16 workgroups), s 3000/16, c 2000/64, d 2000/4 (register kernel,
# 95 - 251 workgroups), z 2048/200 (generic)
RACE_CASES = [("d", 4096, 128, 1), ("s", 3000, 16, 2), ("c", 2000, 64, 3), ("d", 2000, 4, 4), ("z", 2048, 200, 5)]
# generic kernel for s, d, c and the batched back-transformation at d / 128
GENERIC_CASES = [("s", 300, 16, 6), ("d", 517, 128, 7), ("c", 260, 64, 8), ("s", 385, 128, 9), ("d", 700, 3, 10)]


@pytest.mark.fresh_parent
def test_b2t_configuration_children(td, tmp_path):
    """Three child processes one after another (the launch settings are read once per process):
    1. default settings;
    2. DLAF_MI355X_B2T_WORKGROUPS=1: one workgroup runs every sweep in order, so d, e and v must equal the default
       child's bit for bit -- the arithmetic of a sweep does not depend on which workgroup runs it, any difference is a
       hand-off race;
    3. DLAF_MI355X_B2T_KERNEL=generic DLAF_MI355X_BT_FUSED=0: the generic kernel for s, d, c and the batched
       back-transformation for d at band 128, held to the checkers.
    This process does not open the GPU."""
    def child(name, cases, bt_k, **env):
        path = str(tmp_path / f"{name}.npz")
        src = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "cases": cases, "path": path,
                       "keep_v": 800, "bt_k": bt_k}
        r = subprocess.run([sys.executable, "-c", src], cwd=ROOT, env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0 and "CHILD DONE" in r.stdout, (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        return np.load(path)

    base = child("default", RACE_CASES, ())
    one = child("one_workgroup", RACE_CASES, (), DLAF_MI355X_B2T_WORKGROUPS="1")
    for t, n, band, _ in RACE_CASES:
        key = f"{t}_{n}_{band}"
        for part in ("_d", "_e", "_vhash"):
            a, b = base[key + part], one[key + part]
            diff = np.flatnonzero(a != b)
            assert diff.size == 0, (key + part, "differs first at", int(diff[0]), int(diff.size))
    gen = child("generic", GENERIC_CASES, (1, 65), DLAF_MI355X_B2T_KERNEL="generic", DLAF_MI355X_BT_FUSED="0")
    for t, n, band, seed in GENERIC_CASES:
        key = f"{t}_{n}_{band}"
        a0 = random_band(n, band, DT[t], seed)
        d, e, v = gen[key + "_d"], gen[key + "_e"], gen[key + "_v"]
        check(td, a0, band, d, e, v, ("generic", key))
        ldt = np.clongdouble if np.dtype(DT[t]).kind == "c" else np.longdouble
        for k in (1, 65):
            rng = np.random.default_rng(n + k)
            e0 = rng.uniform(-1, 1, (n, k))
            if np.dtype(DT[t]).kind == "c":
                e0 = e0 + 1j * rng.uniform(-1, 1, (n, k))
            ref = td.apply_q(v.astype(ldt), band, e0.astype(DT[t]).astype(ldt))
            err = float(np.abs(gen[key + f"_bt{k}"] - ref).max())
            assert err <= 20 * n * td.error_of(DT[t]), (key, k, err)
