"""CPU half of test_gpu_cholesky_hard.py: the inputs of hard_spd.py are what they claim, the recorded bars are 4 x what
LAPACK reaches on them, the blocked algorithm with inverted 64-column diagonal blocks (emulated in numpy, in the working
precision) stays inside those bars, and every checker fails on an injected fault."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hard_spd as h  # noqa: E402

TYPES = "sdcz"
INPUTS = [(name, t, n, nb) for t in TYPES for (n, nb) in h.sizes_of(t) for name in h.FAMILIES]
PLANTED_600 = [(0,), (63,), (64,), (255,), (256,), (511,), (512,), (599,), (300, 101)]


def emulated(name, t, n, nb):
    low, ws, info = h.emulate_factor(h.family(name, t, n), nb)
    assert low.dtype == h.DT[t] and info == 0
    return low, ws


def factor_passes(t, a, low, info):
    """what every GPU case asserts of a factor: info 0 and both ratios inside the bars"""
    if info != 0:
        return False
    norm, comp = h.factor_ratios(t, a, low)
    return norm <= h.BAR_FACTOR[t][0] and comp <= h.BAR_FACTOR[t][1]


@pytest.mark.parametrize("t", TYPES)
def test_families_have_the_claimed_spectrum(t):
    for n, _ in h.sizes_of(t):
        for name in h.FAMILIES:
            a = h.family(name, t, n)
            assert a.dtype == h.DT[t] and np.array_equal(a, a.conj().T) and not a.flags.writeable
            wide = np.complex128 if t in "cz" else np.float64
            if name == "graded":
                d = h.grading(t, n)
                assert d.max() == 1.0 and d.min() == pytest.approx(10.0 ** h.grading_of(t))
                a = a.astype(wide) / d[:, None] / d[None, :]
            ev = np.linalg.eigvalsh(a.astype(wide))[::-1]
            claim = np.sort(h.spectrum_of(name, t, n))[::-1]
            # rounding to the working type moves an eigenvalue by at most ||dA||_2 <= n eps max|A| (graded: of the
            # core, whose entries the scaling carries along exactly as relative perturbations)
            tol = n * h.eps_of(t) * max(1.0, float(np.abs(a).max()))
            assert np.abs(ev - claim).max() <= tol, (name, t, n, np.abs(ev - claim).max(), tol)
            assert ev[0] / ev[-1] == pytest.approx(h.kappa_of(name, t), rel=0.05 if name != "graded" else 0.2)


@pytest.mark.parametrize("t", TYPES)
def test_lapack_factors_every_input_and_the_records_hold(t):
    """info 0 from ?potrf on the final input set, and REF_FACTOR / REF_SOLVE within a factor of two of what is measured
    here (the bars are constants; this guards the inputs and the measures against drifting away from them)"""
    worst = [0.0, 0.0]
    for name, tt, n, _ in INPUTS:
        if tt != t:
            continue
        for uplo in "LU":
            assert h.lapack_factor(name, t, n, uplo)[0] == 0, (name, t, n, uplo)
            worst = [max(x, y) for x, y in zip(worst, h.lapack_factor_ratios(name, t, n, uplo))]
    print(f"LAPACK {t}: normwise {worst[0]:.5f} componentwise {worst[1]:.5f} (recorded {h.REF_FACTOR[t]})")
    for got, rec in zip(worst, h.REF_FACTOR[t]):
        assert rec / 2 <= got <= 2 * rec
    if t in "dz":
        sol = max(h.lapack_solve_ratio(name, t, n, nrhs, uplo) for n, _ in h.SOLVE_SIZES for name in h.SOLVE_FAMILIES
                  for nrhs in h.NRHS for uplo in "LU")
        print(f"LAPACK {t}: solve {sol:.5f} (recorded {h.REF_SOLVE[t]})")
        assert h.REF_SOLVE[t] / 2 <= sol <= 2 * h.REF_SOLVE[t]
    assert h.BAR_FACTOR[t] == [4 * r for r in h.REF_FACTOR[t]]
    assert all(h.BAR_SOLVE[x] == 4 * h.REF_SOLVE[x] for x in "dz")


@pytest.mark.parametrize("name,t,n,nb", INPUTS)
def test_inverted_block_algorithm_stays_inside_the_bars(name, t, n, nb):
    """were the bars tighter than the algorithm allows, the GPU tests would assert LAPACK, not correctness (the upper
    variant is the same computation on the adjoint)"""
    low, ws = emulated(name, t, n, nb)
    norm, comp = h.factor_ratios(t, h.family(name, t, n), low)
    print(f"emulation {name} {t} n={n} nb={nb}: {norm:.4f} {comp:.4f} (bars {h.BAR_FACTOR[t]})")
    assert norm <= h.BAR_FACTOR[t][0] and comp <= h.BAR_FACTOR[t][1]
    assert h.diagonal_ok(low)
    if t in "dz" and name in h.SOLVE_FAMILIES and (n, nb) in h.SOLVE_SIZES:
        for nrhs in h.NRHS:
            b = h.rhs(t, n, nrhs)
            r = h.solve_ratio(t, h.family(name, t, n), b, h.emulate_solve(low, ws, nb, b))
            print(f"emulated solve nrhs={nrhs}: {r:.4f} (bar {h.BAR_SOLVE[t]})")
            assert r <= h.BAR_SOLVE[t]


# ------------------------------------------------------------------------------------------------- injected faults
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", ["geo", "one_small"])
def test_a_slab_left_out_of_one_tile_is_caught(name, t):
    n, nb = 515, 128
    a = h.family(name, t, n)
    assert factor_passes(t, a, *h.emulate_factor(a, nb)[::2])
    # (tile row, tile column, 64-column block): off the diagonal, the ragged last tile, a diagonal tile
    for fault in (("slab", 3, 2, 1), ("slab", 4, 4, 6), ("slab", 1, 1, 0)):
        low, _, info = h.emulate_factor(a, nb, fault)
        assert not factor_passes(t, a, low, info), fault


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", ["geo", "one_small"])
def test_a_panel_block_with_w_for_its_adjoint_is_caught(name, t):
    n, nb = 515, 128
    a = h.family(name, t, n)
    # (tile row, 64-column block): a whole tile below, the ragged last tile, the rest of the block's own tile
    for fault in (("w", 2, 0), ("w", 4, 5), ("w", 1, 2)):
        low, _, info = h.emulate_factor(a, nb, fault)
        assert not factor_passes(t, a, low, info), fault


@pytest.mark.parametrize("t", "dz")
def test_one_entry_off_by_2_to_the_minus_20_is_caught(t):
    """2^-20 relative is 2^32 units of roundoff in d / z (in s / c it is 8 of them: below any residual bar)"""
    n = 515
    a = h.family("one_small", t, n)
    low = np.array(h.lapack_factor("one_small", t, n, "L")[1])
    good = h.factor_ratios(t, a, low)
    assert good[0] <= h.BAR_FACTOR[t][0] and good[1] <= h.BAR_FACTOR[t][1]
    for i, j in ((300, 300), (514, 514), (0, 0)):
        bad = low.copy()
        bad[i, j] *= 1 + 2.0 ** -20
        norm, comp = h.factor_ratios(t, a, bad)
        assert norm > h.BAR_FACTOR[t][0] and comp > h.BAR_FACTOR[t][1], (i, j, norm, comp)
    # the solve measure sees a wrong solution
    b = h.rhs(t, n, 7)
    x = np.linalg.solve(a, b)
    assert h.solve_ratio(t, a, b, x) <= h.BAR_SOLVE[t]
    x[100, 3] *= 1 + 2.0 ** -20
    assert h.solve_ratio(t, a, b, x) > h.BAR_SOLVE[t]


def test_info_sentinel_and_bit_checkers_fail_on_faults():
    # info off by one: the reference tells neighbouring columns apart and the GPU tests compare with ==, so a driver
    # that reports the column before or after the failing one is refused
    a = h.planted("d", 600, (256,))
    infos = [h.unblocked_info(h.planted("d", 600, (j,))) for j in (255, 256, 257)]
    assert infos == [256, 257, 258]
    for uplo in "LU":
        buf0, _ = h.padded(a)
        assert h.untouched(buf0.copy(), buf0, uplo)
        for where in ((601, 17), (600, 0), (602, 599), (3, 400) if uplo == "L" else (400, 3)):
            buf = buf0.copy()
            buf[where] = np.nextafter(buf[where], 0.0)
            assert not h.untouched(buf, buf0, uplo), (uplo, where)
        inside = buf0.copy()
        inside[(400, 3) if uplo == "L" else (3, 400)] = 1.0
        inside[5, 5] = 1.0
        assert h.untouched(inside, buf0, uplo)
    # -0.0 for 0.0, a NaN for itself: bits, not values
    z = np.zeros((4, 4))
    assert not h.same_bits(z, -z) and h.same_bits(np.full(3, np.nan), np.full(3, np.nan))
    # one bit flipped in the factor a reused handle returns
    low = np.asfortranarray(h.lapack_factor("geo", "d", 129, "L")[1])
    for uplo, (i, j) in (("L", (100, 7)), ("U", (7, 100)), ("L", (128, 128))):
        fac = low if uplo == "L" else np.asfortranarray(low.T)
        flipped = fac.copy()
        flipped.view(np.uint64)[i, j] ^= np.uint64(1)
        assert h.tri_same_bits(fac.copy(), fac, uplo) and not h.tri_same_bits(flipped, fac, uplo)
        other = fac.copy()
        other[j, i] = 5.0 if i != j else other[j, i]
        assert h.tri_same_bits(other, fac, uplo)
    assert not h.diagonal_ok(np.diag([1.0, -1.0])) and not h.diagonal_ok(np.diag([1.0, 1.0 + 1e-30j]))
    assert not h.diagonal_ok(np.diag([1.0, np.nan])) and h.diagonal_ok(np.diag([1.0, 2.0 + 0j]))


# ------------------------------------------------------------------------------------------ not positive definite
def indefinite_cases(t):
    yield "planted 515/514", h.planted(t, 515, (514,)), 515
    for where in PLANTED_600:
        yield f"planted {where}", h.planted(t, 600, where), min(where) + 1
    for where in h.THROUGH_SHAPE:
        yield f"through {where}", h.through_updates(t, where), None


@pytest.mark.parametrize("t", TYPES)
def test_indefinite_cases_are_decisive_and_agree_with_lapack(t):
    import scipy.linalg as sl
    for label, a, expect in indefinite_cases(t):
        info = h.unblocked_info(a)
        if expect is not None:
            assert info == expect, (label, info)
        else:
            lo, hi = h.THROUGH_RANGE[label.split()[1]]
            assert lo < info <= hi, (label, info)
            assert (np.diagonal(a).real > 0).all()
            ev = np.linalg.eigvalsh(a.astype(np.complex128))
            assert ev[0] == pytest.approx(-0.5, abs=1e-3) and 1 - 1e-3 <= ev[1] and ev[-1] <= 2 + 1e-3
        assert h.decisive(a), label
        for lower in (True, False):
            assert sl.lapack.get_lapack_funcs("potrf", (a,))(a, lower=lower)[1] == info, (label, lower)


@pytest.mark.parametrize("t", "dz")
def test_unblocked_info_on_nan_and_inf(t):
    a = h.family("one_small", t, 600)
    assert h.unblocked_info(a) == 0
    for j in h.NONFINITE_DIAG:
        assert h.unblocked_info(h.with_value(a, j, j, np.nan)) == j + 1
    for i, j in h.NONFINITE_OFF:
        assert h.unblocked_info(h.with_value(a, i, j, np.nan)) == i + 1
        assert h.unblocked_info(h.with_value(a, i, j, np.inf)) == i + 1


# --------------------------------------------------------------------------------------------- scale equivariance
@pytest.mark.parametrize("t", TYPES)
def test_scaled_inputs_stay_in_the_normal_range(t):
    from oracle import oracle
    oracle.lib()
    import scipy.linalg as sl
    k = h.scale_exponent(t)
    for a in (oracle.set_random_hpd(515, 128, h.DT[t]), h.family("geo", t, 515)):
        c, info = sl.lapack.get_lapack_funcs("potrf", (a,))(a, lower=True, clean=True)
        assert info == 0
        for sign in (1, -1):
            assert h.in_normal_range(a, t, 2 * sign * k) and h.in_normal_range(c, t, sign * k)
            s = h.scaled(a, sign * k)
            assert s.dtype == a.dtype and np.isfinite(s).all()
            assert h.same_bits(h.scaled(s, -sign * k), np.asfortranarray(a))  # the scaling is exact
            cs, info = sl.lapack.get_lapack_funcs("potrf", (s,))(s, lower=True, clean=True)
            assert info == 0 and h.in_normal_range(cs, t, 0)
    assert not h.in_normal_range(np.array([1.0, 1e-300]), "d", -200) and not h.in_normal_range(np.array([1.0]), "s", 128)
