"""GPU parity tests of generalized_to_standard through the C ABI: the reference's own test
(test/unit/eigensolver/test_gen_to_std.cpp:54-83: analytic operands, abs tolerance 10 (m+1) error, factor
untouched) plus random operands against the oracle restatement of GenToStd::call_L.

The random operands above are A = B / n (the generator is deterministic), so their exact result is I / n and the absolute
tolerance sees the diagonal only; the analytic operands decay as 2^-(i+j).  The "coupled" tests below run operands whose
off-diagonal result is of order one (tests/hegst_cases.py: A uniform Hermitian, B = G G^H / n + 2 I, the factor rounded
once from the wide type, the reference C = L^-1 A L^-H in the wide type from that rounded factor) and compare EVERY element
of the uplo triangle: ratio = max |got - C| / (u |L^-1| |A| |L^-H|) <= 16 max(rho_ref, 4), rho_ref the same ratio of the
oracle's restatement in the working precision.  The other triangle of A and the whole factor buffer must come back bit for
bit.  Entries: the host entry, p?potrf -> p?hegst and the resident DeviceMatrix chain (the reference built from the factor
the library returned), and for d / z the DLAF_MI355X_HEGST_LOOKAHEAD=1 child.  tests/test_hegst_cases.py is the CPU half:
an emulation of the two phases passes the same check and fails it with each of six faults injected.

Observed on one MI355X, ratio / rho_ref (uplo L and U give the same figures; the lookahead child gives the host entry's):

    shape        d host      d p?hegst   z host     z p?hegst  s host      s p?hegst   c host     c p?hegst
    129 /  64    2.52/ 9.40  2.23/ 9.28  2.40/3.80  2.36/3.85  3.50/ 8.08  3.58/ 7.17  4.38/3.51  4.37/3.27
    200 /  64    2.71/ 6.67  2.77/ 6.73  3.04/4.27  3.15/3.85  4.65/10.61  4.36/ 9.01  4.94/4.04  3.99/4.30
    300 / 128   27.97/ 8.85 28.86/ 9.29  2.76/5.02  2.58/4.84  3.74/ 9.19  4.74/ 9.27  4.67/4.92  4.80/4.77
    600 / 256   28.84/12.47 28.96/12.49  2.90/5.41  2.77/5.40  4.14/11.62  4.69/12.65  4.64/6.13  4.54/6.22
    600 / 512    5.31/12.47  4.94/12.49  2.90/5.22  2.77/5.40

(the resident chain gives the p?hegst figures: the same factor, the same result).  The largest ratio against its bar is
27.97 against 141.6 (d, 300 / 128).  The 28 of d at nb = 128 and 256 sits in the full off-diagonal tiles of a block column
and comes from the fp64 interior path of the update kernel, which loads C into the MFMA accumulators and subtracts the
K = nb products of a half-hemm from it one by one: every step rounds at the size of C (0.3), not of the products (0.002).
A numpy model of that order on the (1, 0) tile of 300 / 128 gives an error of mean 2.50 u, max 29.2 u, the GPU 2.52 u and
28.6 u; summed apart and subtracted once it is 0.28 u and 1.6 u.  Both are inside the gamma_K (|C| + |A||B|) bound of a
GEMM and inside the bar; the ragged tiles, nb = 64 / 512 (no full interior block) and the other types take the epilogue
that sums apart.  On the grids (tests/dist_worker.py, rank 0) d L 530 / 64 and z U 300 / 32 run the same check:
2 x 2, d L from source rank (1, 1) 3.24 / 8.87, z U 2.80 / 4.09."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hegst_cases as hc

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
# the coupled operands of tests/hegst_cases.py in the same child process, behind the cases above
COUPLED_SHAPES = [(129, 64), (200, 64), (300, 128), (600, 256), (600, 512)]
COUPLED = [(t, uplo, n, nb) for t in TYPES for uplo in ("L", "U") for n, nb in (COUPLED_SHAPES if t in "dz" else COUPLED_SHAPES[:4])]
LOOKAHEAD_COUPLED = [c for c in COUPLED if c[0] in "dz"]
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
    fac = np.asfortranarray(ops[f"f{i}"])
    info = dl.generalized_to_standard(grid, uplo, got, fac, nb)
    assert info == 0, (t, uplo, n, nb, info)
    out[f"g{i}"] = got
    out[f"l{i}"] = fac
np.savez(%r, **out)
print("DONE", flush=True)
"""


def test_gen_to_std_lookahead_vs_oracle(oracle, tmp_path):
    """DLAF_MI355X_HEGST_LOOKAHEAD=1 (read when the reduction starts; set for a child process so that no other test sees
    it): the diagonal tile / panel chain on a side stream beside a persistent trailing update.  Same operands, bound and
    untouched-triangle check as test_gen_to_std_random_vs_oracle.  The same child then runs the coupled operands of
    tests/hegst_cases.py (d / z, every shape, both uplo), checked as in test_gen_to_std_coupled_host_entry."""
    cases = [random_case(oracle, *c) for c in LOOKAHEAD_CASES]
    coupled = [(hc.coupled_case(t, n, hc.seed_of(n)), uplo, nb) for t, uplo, n, nb in LOOKAHEAD_COUPLED]
    operands = [(c[0], c[1]) for c in cases] + [(hc.a_operand(c, uplo), hc.factor_operand(c, uplo)) for c, uplo, _ in coupled]
    ops_path, out_path = str(tmp_path / "operands.npz"), str(tmp_path / "results.npz")
    np.savez(ops_path, **{f"a{i}": c[0] for i, c in enumerate(operands)}, **{f"f{i}": c[1] for i, c in enumerate(operands)})
    r = subprocess.run([sys.executable, "-c", LOOKAHEAD_CHILD % (ROOT, ops_path, LOOKAHEAD_CASES + LOOKAHEAD_COUPLED, out_path)],
                       cwd=ROOT, env=dict(os.environ, DLAF_MI355X_HEGST_LOOKAHEAD="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    res = np.load(out_path)
    for i, ((t, uplo, n, nb), (a0, fac, ref)) in enumerate(zip(LOOKAHEAD_CASES, cases)):
        check_random_case(oracle, t, uplo, n, nb, a0, ref, res[f"g{i}"])
    failed = []
    for i, (case, uplo, nb) in enumerate(coupled, start=len(cases)):
        assert hc.same_bits(res[f"l{i}"], operands[i][1]), ("the factor changed", case.t, uplo, case.n, nb)
        ok, msg = hc.verdict(res[f"g{i}"], case, uplo, nb, hc.rho_ref(oracle, case, uplo, nb), "lookahead")
        if not ok:
            failed.append(msg)
    assert not failed, failed


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


# ---- operands with real coupling, at roundoff level (tests/hegst_cases.py) --------------------------------------------
def coupled_id(c):
    return f"{c[0]}{c[1]}-{c[2]}-{c[3]}"


@pytest.mark.parametrize("t,uplo,n,nb", COUPLED, ids=[coupled_id(c) for c in COUPLED])
def test_gen_to_std_coupled_host_entry(dlaf, grid, oracle, t, uplo, n, nb):
    case = hc.coupled_case(t, n, hc.seed_of(n))
    a_in, fac_in = hc.a_operand(case, uplo), hc.factor_operand(case, uplo)
    got, fac = a_in.copy(order="F"), fac_in.copy(order="F")
    assert dlaf.generalized_to_standard(grid, uplo, got, fac, nb) == 0
    assert hc.same_bits(fac, fac_in), "the factor buffer changed"
    hc.check(got, case, uplo, nb, hc.rho_ref(oracle, case, uplo, nb), "host entry")


@pytest.mark.parametrize("t,uplo,n,nb", COUPLED, ids=[coupled_id(c) for c in COUPLED])
def test_gen_to_std_coupled_pxhegst_and_resident_chain(dlaf, grid, oracle, t, uplo, n, nb):
    """p?potrf -> p?hegst and the same chain on resident matrices.  The factor is the library's own: the reference
    C = L^-1 A L^-H is built from the factor it returned, rho_ref from the oracle on that factor."""
    base = hc.coupled_case(t, n, hc.seed_of(n))
    a_in, b_in = hc.a_operand(base, uplo), hc.b_operand(base, uplo)
    desc = [1, grid.context, n, n, nb, nb, 0, 0, n]
    fac = b_in.copy(order="F")
    assert dlaf.pxpotrf(uplo, n, fac, 1, 1, desc) == 0
    case = base.with_factor(fac, uplo)
    rho = hc.rho_ref(oracle, case, uplo, nb)
    got, fac_io = a_in.copy(order="F"), fac.copy(order="F")
    assert dlaf.pxhegst(1, uplo, n, got, 1, 1, desc, fac_io, 1, 1, desc) == (1.0, 0)
    assert hc.same_bits(fac_io, fac), "the factor buffer changed"
    hc.check(got, case, uplo, nb, rho, "p?hegst")
    # resident: upload A and B once, factor, reduce, download
    dt = oracle.DTYPES[t]
    am, bm = dlaf.DeviceMatrix(grid, dt, uplo, n, nb), dlaf.DeviceMatrix(grid, dt, uplo, n, nb)
    try:
        am.upload(a_in)
        bm.upload(b_in)
        assert bm.factorize() == 0
        assert am.generalized_to_standard(bm) == 0
        out, fac_res = a_in.copy(order="F"), b_in.copy(order="F")
        am.download(out)
        bm.download(fac_res)
    finally:
        am.close()
        bm.close()
    if not hc.same_bits(fac_res, fac):   # another factor than p?potrf's: its own reference
        case = base.with_factor(fac_res, uplo)
        rho = hc.rho_ref(oracle, case, uplo, nb)
    hc.check(out, case, uplo, nb, rho, "resident")
