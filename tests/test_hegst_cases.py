"""No GPU.  The CPU half of the coupled gen_to_std tests (tests/hegst_cases.py): the numpy emulation of the two phases
of csrc/host/gen_to_std.cpp, in the working precision, goes through the checker the GPU results go through.  It must stay
below the bar 16 max(rho_ref, 4) on every case of the GPU tests and leave it with each one of these faults injected: the
second segment L_ik A_jk^H dropped from one trailing tile, step (4) omitted for one column, one Phase II
A(i, c) -= L_ij R_j dropped, 0.5 D replaced by D in one step, one stale (pre-update) A tile read by a panel step and,
for c / z, the Phase II back-transposition done without the conjugate.

test_old_operands_pass_a_missing_conjugate records why the operands had to change: with A = B / n (what random_case of
tests/test_gpu_gen_to_std.py builds) the exact result is I / n and the old check passes a result whose Phase II
back-transposition lost its conjugate."""
import numpy as np
import pytest

import hegst_cases as hc
from test_gpu_gen_to_std import check_random_case, random_case

SHAPES = [(129, 64), (200, 64), (300, 128), (600, 256), (600, 512)]
CASES = [(t, n, nb) for t in "dzsc" for n, nb in (SHAPES if t in "dz" else SHAPES[:4])]


@pytest.mark.parametrize("t,n,nb", CASES)
def test_emulation_passes_the_bar_and_every_fault_fails(oracle, t, n, nb):
    case = hc.coupled_case(t, n, hc.seed_of(n))
    for uplo in ("L", "U"):
        a_in, fac = hc.a_operand(case, uplo), hc.factor_operand(case, uplo)
        fac0 = fac.copy(order="F")
        rho = hc.rho_ref(oracle, case, uplo, nb)
        assert 0 < rho < 64, rho     # the reference itself sits at roundoff level: the bar is no licence
        hc.check(hc.emulate(a_in, fac, uplo, nb), case, uplo, nb, rho, "emulation")
        assert np.array_equal(fac, fac0)
        for fault in hc.FAULTS:
            if not hc.fault_applies(fault, t, n, nb):
                continue
            got = hc.emulate(a_in, fac, uplo, nb, fault)
            r = hc.ratio(got, case, uplo)
            ok, _ = hc.verdict(got, case, uplo, nb, rho, f"fault {fault}")
            assert not ok, (fault, t, uplo, n, nb, r)
            # no near miss: a lost term of a sum is of the order of mag itself, 1 / u times the unit of the ratio, and
            # even in single precision and in the one-row tile of n = 129 that is three orders above the bar
            assert r > 1e3 * hc.bar(rho), (fault, t, uplo, n, nb, r)


def test_every_fault_runs_somewhere():
    for fault in hc.FAULTS:
        for t in ("cz" if fault == "noconj" else "dzsc"):
            assert any(hc.fault_applies(fault, tt, n, nb) for tt, n, nb in CASES if tt == t), (fault, t)


def test_checker_sees_the_other_triangle_and_nonfinite_results(oracle):
    case = hc.coupled_case("s", 129, hc.seed_of(129))
    rho = hc.rho_ref(oracle, case, "L", 64)
    good = hc.emulate(hc.a_operand(case, "L"), hc.factor_operand(case, "L"), "L", 64)
    assert hc.verdict(good, case, "L", 64, rho, "emulation")[0]
    bad = good.copy()
    bad[0, 128] = 0
    assert not hc.verdict(bad, case, "L", 64, rho, "other triangle")[0]
    bad = good.copy()
    bad[128, 0] = np.nan
    assert not hc.verdict(bad, case, "L", 64, rho, "nan")[0]


@pytest.mark.parametrize("t", ["c", "z"])
def test_old_operands_pass_a_missing_conjugate(oracle, t):
    """A = B / n: the exact result is I / n, the off-diagonal part of the result is far below the absolute tolerance of
    check_random_case, and a Phase II without its conjugate passes the old check."""
    uplo, n, nb = "L", 300, 64
    a0, fac, ref = random_case(oracle, t, uplo, n, nb)
    off = np.abs(np.tril(ref, -1)).max()
    tol = 10 * (n + 1) * 8 * oracle.eps_of(oracle.DTYPES[t])
    print(f"{t}: largest off-diagonal entry of the oracle's result {off:.2e}, the old tolerance {tol:.2e}")
    assert off < 1e-3 * tol
    got = hc.emulate(a0, fac, uplo, nb, "noconj")
    check_random_case(oracle, t, uplo, n, nb, a0, ref, got)     # the old check passes the fault
