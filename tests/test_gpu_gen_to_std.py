"""GPU parity tests of generalized_to_standard through the C ABI: the reference's own test
(test/unit/eigensolver/test_gen_to_std.cpp:54-83: analytic operands, abs tolerance 10 (m+1) error, factor
untouched) plus random operands against the oracle restatement of GenToStd::call_L."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TYPES = ["d", "z", "s", "c"]
SIZES = [(0, 2), (5, 8), (34, 34), (4, 3), (16, 10), (34, 13), (32, 5)]  # test_gen_to_std.cpp:54-58


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def grid(dlaf):
    return dlaf.Grid.single()


def err_of(orc, t):
    return (8 if t in "cz" else 2) * orc.eps_of(orc.DTYPES[t])


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_gen_to_std_local_analytic(dlaf, grid, oracle, t, uplo):
    dt = oracle.DTYPES[t]
    for m, mb in SIZES + [(150, 64), (200, 70), (300, 128)]:
        tmat, a, b = oracle.gen_to_std_setters(uplo, m, dt)
        got = a.copy(order="F")
        fac = tmat.copy(order="F")
        assert dlaf.generalized_to_standard(grid, uplo, got, fac, mb) == 0
        ok, md = oracle.check_near(b, got, 0, 10 * (m + 1) * err_of(oracle, t))  # includes the -9.9 triangle
        assert ok, (m, mb, md)
        assert np.array_equal(fac, tmat)   # CHECK_MATRIX_NEAR(el_t, mat_th, 0, error) of the distributed test


_RANDOM_CASES = {}


def random_case(oracle, t, uplo, n, nb):
    """(A, the Cholesky factor of B, the oracle's result) of one random case; computed once, never written to"""
    key = (t, uplo, n, nb)
    if key not in _RANDOM_CASES:
        dt = oracle.DTYPES[t]
        b0 = oracle.set_random_hpd(n, nb, dt)
        a0 = (oracle.set_random_hpd(n, nb, dt) * dt(1.0 / n)).astype(dt)
        fac = b0.copy(order="F")
        assert oracle.cholesky_local(uplo, fac, nb) == 0
        ref = a0.copy(order="F")
        oracle.gen_to_std_local(uplo, ref, fac, nb)
        _RANDOM_CASES[key] = (a0, fac, ref)
    return _RANDOM_CASES[key]


def check_random_case(oracle, t, uplo, n, nb, a0, ref, got):
    scale = np.abs(oracle.tri(uplo, ref)).max()
    tol = 10 * (n + 1) * err_of(oracle, t) * max(1.0, scale)
    ok, md = oracle.check_near(oracle.tri(uplo, ref), oracle.tri(uplo, got), 0, tol)
    assert ok, (t, uplo, n, nb, md, tol)
    other = np.triu(got, 1) if uplo == "L" else np.tril(got, -1)
    assert np.array_equal(other, np.triu(a0, 1) if uplo == "L" else np.tril(a0, -1))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_gen_to_std_random_vs_oracle(dlaf, grid, oracle, t, uplo):
    # (the numpy restatement of GenToStd::call_L is what takes the time: 1536 instead of 2048 for the nb = 512 case)
    for n, nb in [(300, 64), (515, 128), (1024, 256), (129, 64), (1536 if t == "d" else 512, 512 if t == "d" else 256)]:
        a0, fac, ref = random_case(oracle, t, uplo, n, nb)
        got = a0.copy(order="F")
        assert dlaf.generalized_to_standard(grid, uplo, got, fac.copy(order="F"), nb) == 0
        check_random_case(oracle, t, uplo, n, nb, a0, ref, got)


LOOKAHEAD_CASES = [(t, uplo, n, nb) for t in ("d", "z") for uplo in ("L", "U")
                   for n, nb in [(300, 64), (515, 128), (1024, 256)]]
LOOKAHEAD_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
import dla_future_amd as dl
dl.initialize()
grid = dl.Grid.single()
ops = np.load(%r)
out = {}
for i, (t, uplo, n, nb) in enumerate(%r):
    got = np.asfortranarray(ops[f"a{i}"])
    info = dl.generalized_to_standard(grid, uplo, got, np.asfortranarray(ops[f"f{i}"]), nb)
    assert info == 0, (t, uplo, n, nb, info)
    out[f"g{i}"] = got
np.savez(%r, **out)
print("DONE", flush=True)
"""


def test_gen_to_std_lookahead_vs_oracle(oracle, tmp_path):
    """DLAF_MI355X_HEGST_LOOKAHEAD=1 (read when the reduction starts; set for a child process so that no other test sees
    it): the diagonal tile / panel chain on a side stream beside a persistent trailing update.  Same operands, bound and
    untouched-triangle check as test_gen_to_std_random_vs_oracle."""
    cases = [random_case(oracle, *c) for c in LOOKAHEAD_CASES]
    ops_path, out_path = str(tmp_path / "operands.npz"), str(tmp_path / "results.npz")
    np.savez(ops_path, **{f"a{i}": c[0] for i, c in enumerate(cases)}, **{f"f{i}": c[1] for i, c in enumerate(cases)})
    r = subprocess.run([sys.executable, "-c", LOOKAHEAD_CHILD % (ROOT, ops_path, LOOKAHEAD_CASES, out_path)], cwd=ROOT,
                       env=dict(os.environ, DLAF_MI355X_HEGST_LOOKAHEAD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    res = np.load(out_path)
    for i, ((t, uplo, n, nb), (a0, fac, ref)) in enumerate(zip(LOOKAHEAD_CASES, cases)):
        check_random_case(oracle, t, uplo, n, nb, a0, ref, res[f"g{i}"])


def test_pdhegst_scalapack_entry_and_device_handles(dlaf, grid, oracle):
    n, nb = 260, 64
    for t in ("d", "z"):
        dt = oracle.DTYPES[t]
        b0 = oracle.set_random_hpd(n, nb, dt)
        a0 = (oracle.set_random_hpd(n, nb, dt) * dt(1.0 / n)).astype(dt)
        fac = b0.copy(order="F")
        assert dlaf.pxpotrf("L", n, fac, 1, 1, [1, grid.context, n, n, nb, nb, 0, 0, n]) == 0
        ref = a0.copy(order="F")
        oracle.gen_to_std_local("L", ref, fac, nb)
        got = a0.copy(order="F")
        desc = [1, grid.context, n, n, nb, nb, 0, 0, n]
        scale, info = dlaf.pxhegst(1, "L", n, got, 1, 1, desc, fac, 1, 1, desc)
        assert (scale, info) == (1.0, 0)
        tol = 10 * (n + 1) * err_of(oracle, t) * max(1.0, np.abs(np.tril(ref)).max())
        assert oracle.check_near(np.tril(ref), np.tril(got), 0, tol)[0]
        # p?potrf -> gen_to_std chained on device-resident matrices
        am = dlaf.DeviceMatrix(grid, dt, "L", n, nb)
        bm = dlaf.DeviceMatrix(grid, dt, "L", n, nb)
        am.upload(a0)
        bm.upload(b0)
        assert bm.factorize() == 0
        assert am.generalized_to_standard(bm) == 0
        out = a0.copy(order="F")
        am.download(out)
        assert oracle.check_near(np.tril(ref), np.tril(out), 0, tol)[0]
        am.close()
        bm.close()
