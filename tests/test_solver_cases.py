"""No GPU.  The CPU half of test_triangular_solver_uniform_componentwise_bound (tests/test_gpu_solver.py): on the operands
and with the checker of tests/solver_cases.py the oracle's generic trsm stays inside the component-wise residual bound
for every type, shape, side / uplo / op / diag, and a solve with one off-diagonal tile of the triangular matrix dropped
leaves it -- in complex float too, where the absolute tolerance 40 (m + 1) err of the random cases lets such a solve
pass (a dropped tile moves the result by 0.66 - 6 times that tolerance)."""
import pytest

import solver_cases as sc


@pytest.mark.parametrize("t", ["s", "d", "c", "z"])
def test_oracle_trsm_is_inside_the_bound_and_a_dropped_tile_is_not(oracle, t):
    alpha = sc.alpha_of(t)
    worst, least_fault = 0.0, float("inf")
    for (m, n, nb), side, uplo, op, diag in sc.VARIANTS:
        a, b = sc.triangle(t, m if side == "L" else n, uplo), sc.rhs(t, m, n)
        x = b.copy(order="F")
        oracle.trsm(side, uplo, op, diag, alpha, a, x)
        r, where = sc.residual_ratio(t, side, uplo, op, diag, alpha, a, b, x)
        assert r <= 1, (t, m, n, nb, side, uplo, op, diag, r, where)
        worst = max(worst, r)
        x = b.copy(order="F")
        oracle.trsm(side, uplo, op, diag, alpha, sc.drop_tile(a, uplo, nb), x)
        r, where = sc.residual_ratio(t, side, uplo, op, diag, alpha, a, b, x)
        assert r > 100, (t, m, n, nb, side, uplo, op, diag, r, where)
        least_fault = min(least_fault, r)
    print(f"{t}: oracle trsm max |residual| / bound = {worst:.3f}; dropped tile: at least {least_fault:.3g}")
    assert worst > 0
