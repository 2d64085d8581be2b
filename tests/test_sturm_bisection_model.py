"""The Sturm-count / bisection kernels (csrc/device/kernels_sturm.hip) as a numpy model, and the checker the GPU tests
share.  No GPU.

Emulation.  `prepare`, `count_scaled` and `bisect` repeat the three kernels in IEEE double, operation for operation and
in the kernels' order.  The kernels are compiled with floating-point contraction off and divide with the correctly
rounded IEEE division, so the model uses no fma: numpy's -, *, / on float64 are the same functions.  (`lo + (hi - lo) *
0.5` and the products with powers of two are exact scalings; min / max reductions do not depend on their order.)

Referee.  Sturm counts of T - sigma I in wider arithmetic on the matrix as given (a float32 or float64 matrix is exact
in both): mpmath at 160 bits where it is importable and n <= MPMATH_MAX_N, np.longdouble otherwise.  The limit is one of
cost alone: a count is n dependent mpmath divisions (10 us each in pure Python), the checker needs 2 n of them, and at
n = 777 that is 10 s for one matrix.  np.longdouble's unit roundoff 2^-64 is 2^11 below double's, so by the same
argument as below its own error is tol / 2000.  Matrices whose spectrum is known in closed form are refereed by that
spectrum instead (`spectrum_referee`).

The check.  For every computed w_j:  count_ref(w_j - tol_j) <= j  and  count_ref(w_j + tol_j) >= j + 1, that is
lambda_j in (w_j - tol_j, w_j + tol_j], with

    tol_j = stopping width + c eps max(|gl|, |gu|) 2^k + rounding of w_j to its type,

  stopping width = max(pivmin 2^k, 2 eps |w_j|): the bisection ends with hi - lo <= max(pivmin, 2 eps max(|lo|, |hi|))
      (or an interval that cannot be split, which is narrower), w_j is its midpoint, and max(|lo|, |hi|) <= |w_j| (1 + eps);
  eps = 2^-52 (the recurrence runs in double for both types), [gl, gu] the widened Gershgorin interval of the scaled
      matrix, which contains the spectrum, so max(|gl|, |gu|) >= ||T||_2 >= max |e|;
  rounding of w_j: 0 for float64 (the scaling back by 2^k is exact), half an ulp of float32, 2^-24 |w_j|, for float32.

c = 2.5, from the backward error of the recurrence (Kahan 1966; the comments of LAPACK's dstebz / dlaebz).  With
u = eps / 2 the unit roundoff, the computed pivots satisfy
    q_i = [ (d_i - s)(1 + a_i) - (E_{i-1} / q_{i-1}) (1 + b_i) ] (1 + c_i),    |a_i|, |b_i|, |c_i| <= u,
where E = e^2 (1 + f), |f| <= u, is the rounded square.  Dividing by (1 + a_i)(1 + c_i) > 0, the numbers
Q_i = q_i / ((1 + a_i)(1 + c_i)) have the signs of the q_i and satisfy EXACTLY
    Q_i = (d_i - s) - e_{i-1}^2 (1 + f)(1 + b_i) / ((1 + a_i)(1 + a_{i-1})(1 + c_{i-1})) / Q_{i-1}:
they are the pivots of a matrix with the same diagonal and shift whose squared off-diagonal entries are off by at most
5 u relatively, so its off-diagonal entries by 2.5 u, and the symmetric perturbation has 2-norm at most 2 * 2.5 u max|e|
= 2.5 eps max|e|.  By Weyl every eigenvalue moves by at most that: c = 2.5, independent of n.  (The pivmin guard moves a
diagonal entry by less than 2 pivmin ~ 2^-1021 max(1, max e^2): nothing next to eps ||T|| for a matrix that is not zero.)
The count is exact for the perturbed matrix, whatever the shift, so bisection brackets lambda_j of SOME such matrix at
every step; different steps may see different perturbations, all within the same bound.

Observed (this file's matrices, emulation; test_observed_margin prints the figure per matrix).  float64: the check still
passes for every matrix with tol scaled by 2^-2 and fails for some at 2^-3: the worst ratio of the observed error to the
derived bound lies in (1/8, 1/4].  float32: it fails for most matrices at 2^-1, as it must: there tol is in essence the
half ulp of the result's own rounding, which is attained: the worst ratio lies in (1/2, 1].

Fault injection.  The same two checks (`check_counts`, `check_eigenvalues`) must reject the model with each of the
faults of FAULTS injected."""
import bisect

import numpy as np
import pytest

try:
    import mpmath
except ImportError:  # pragma: no cover
    mpmath = None

EPS = 2.0 ** -52
FUDGE = 2.1
DBL_MIN = float(np.finfo(np.float64).tiny)
MAX_ITERATIONS = 1200          # kSturmMaxIterations
C_BACKWARD = 2.5
MPMATH_MAX_N = 300
FAULTS = ("e_for_e2", "no_pivmin_guard", "last_row_skipped", "count_off_by_one", "four_steps_short", "not_scaled_back")


def _ilogb(x: float) -> int:
    return int(np.frexp(x)[1]) - 1


# ------------------------------------------------------------------------------------------------ the model
class Prepared:
    pass


def prepare(d, e):
    """sturm_prepare_kernel: the scaled matrix as doubles, the widened Gershgorin interval, pivmin, k, flag, cap."""
    p = Prepared()
    d64 = np.asarray(d).astype(np.float64)
    e64 = np.asarray(e).astype(np.float64)
    n = p.n = d64.shape[0]
    assert e64.shape[0] == max(n - 1, 0)
    p.bad = not (np.all(np.isfinite(d64)) and np.all(np.isfinite(e64)))
    if p.bad:
        p.k = 0
        return p
    mx = max(np.max(np.abs(d64), initial=0.0), np.max(np.abs(e64), initial=0.0))
    p.k = 0 if mx == 0.0 else _ilogb(mx)
    p.ds = np.ldexp(d64, -p.k)
    p.es = np.ldexp(e64, -p.k)
    p.e2 = p.es * p.es
    el = np.concatenate(([0.0], p.es))
    er = np.concatenate((p.es, [0.0]))
    r = np.abs(el) + np.abs(er)
    gl = np.min(p.ds - r)
    gu = np.max(p.ds + r)
    e2max = np.max(p.e2, initial=0.0)
    p.pivmin = DBL_MIN * max(1.0, e2max)
    tnorm = max(abs(gl), abs(gu))
    t1 = np.float64(FUDGE) * tnorm
    t2 = t1 * EPS
    t3 = t2 * np.float64(n)
    t4 = np.float64(2.0 * FUDGE) * p.pivmin
    wd = t3 + t4
    p.gl = float(gl - wd)
    p.gu = float(gu + wd)
    p.cap = min(max(_ilogb(p.gu - p.gl) - _ilogb(p.pivmin) + 3, 1), MAX_ITERATIONS)
    return p


def count_scaled(p, sigma, fault=None):
    """sturm_count: the number of pivots q <= pivmin of the scaled matrix minus sigma (an array, one lane each)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    q = np.ones_like(sigma)
    cnt = np.zeros(sigma.shape, dtype=np.int64)
    off = np.concatenate(([0.0], p.es if fault == "e_for_e2" else p.e2))
    rows = p.n - 1 if fault == "last_row_skipped" else p.n
    with np.errstate(all="ignore"):
        for i in range(rows):
            tmp = p.ds[i] - sigma
            q = tmp - off[i] / q
            if fault != "no_pivmin_guard":
                q = np.where(np.abs(q) < p.pivmin, -p.pivmin, q)
            cnt += (q < -p.pivmin) if fault == "count_off_by_one" else (q <= p.pivmin)
    return cnt


def sturm_count(d, e, shifts, fault=None):
    """sturm_count_kernel: counts for shifts in the caller's scale; -1 for a matrix that is not finite."""
    p = prepare(d, e)
    shifts = np.asarray(shifts, dtype=np.asarray(d).dtype).astype(np.float64)
    if p.bad:
        return np.full(shifts.shape, -1, dtype=np.int64)
    return count_scaled(p, np.ldexp(shifts, -p.k), fault)


def _bisect(p, begin, end, fault, limit):
    j = np.arange(begin, end)
    lo = np.full(j.shape, p.gl)
    hi = np.full(j.shape, p.gu)
    mid = lo + (hi - lo) * 0.5
    active = np.ones(j.shape, dtype=bool)
    steps = np.zeros(j.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for _ in range(p.cap):
            tol = np.maximum(p.pivmin, (2.0 * EPS) * np.maximum(np.abs(lo), np.abs(hi)))
            active &= ~((mid == lo) | (mid == hi) | (hi - lo <= tol))
            if limit is not None:
                active &= steps < limit
            if not active.any():
                break
            a = np.nonzero(active)[0]
            c = count_scaled(p, mid[a], fault)
            up = c > j[a]
            hi[a[up]] = mid[a[up]]
            lo[a[~up]] = mid[a[~up]]
            mid[a] = lo[a] + (hi[a] - lo[a]) * 0.5
            steps[a] += 1
    return mid, steps


def eigenvalues(d, e, begin=0, end=None, fault=None):
    """sturm_bisect_kernel: w[begin:end] of the matrix d, e in its own type (the other entries are not computed)."""
    dtype = np.asarray(d).dtype
    p = prepare(d, e)
    end = p.n if end is None else end
    if p.bad:
        return np.full(end - begin, np.nan, dtype=dtype)
    mid, steps = _bisect(p, begin, end, fault, None)
    if fault == "four_steps_short":
        mid, _ = _bisect(p, begin, end, None, np.maximum(steps - 4, 0))
    with np.errstate(all="ignore"):
        w = mid if fault == "not_scaled_back" else np.ldexp(mid, p.k)
        return w.astype(dtype)


# ------------------------------------------------------------------------------------------------ the referee
def sturm_referee(d, e):
    """count_ref(x) = the number of eigenvalues <= x of the matrix d, e, in wider arithmetic (module docstring)."""
    d = np.asarray(d)
    e = np.asarray(e)
    n = d.shape[0]
    if mpmath is not None and n <= MPMATH_MAX_N:
        from mpmath.libmp import from_float, mpf_add, mpf_div, mpf_mul, mpf_sign, mpf_sub
        prec = 160
        dm = [from_float(float(x)) for x in d]
        e2 = [mpf_mul(from_float(float(x)), from_float(float(x))) for x in e]   # exact (no precision given)
        tiny = from_float(2.0 ** -1000)
        tiny = mpf_mul(mpf_mul(tiny, tiny), mpf_mul(tiny, tiny))                 # 2^-4000: a zero pivot's stand-in

        def count(x):
            s = x if isinstance(x, tuple) else from_float(float(x))
            q = mpf_sub(dm[0], s, prec, "n")
            c = 0
            for i in range(n):
                if i > 0:
                    q = mpf_sub(mpf_sub(dm[i], s, prec, "n"), mpf_div(e2[i - 1], q, prec, "n"), prec, "n")
                sg = mpf_sign(q)
                if sg <= 0:
                    c += 1
                if sg == 0:
                    q = mpf_sub(from_float(0.0), tiny)
            return c

        count.exact_sum = lambda a, b: mpf_add(from_float(float(a)), from_float(float(b)))   # exact (no precision given)
        return count
    ld = np.longdouble
    dl = d.astype(ld)
    e2l = e.astype(ld) ** 2
    tiny = np.finfo(ld).tiny

    def count_many(x):
        s = np.asarray(x, dtype=ld)
        q = np.ones_like(s)
        c = np.zeros(s.shape, dtype=np.int64)
        with np.errstate(all="ignore"):
            for i in range(n):
                q = (dl[i] - s) - (e2l[i - 1] / q if i > 0 else 0)
                c += q <= 0
                q = np.where(q == 0, -tiny, q)
        return c

    def count(x):
        return int(count_many(np.asarray([x], dtype=ld))[0])

    count.many = count_many
    count.exact_sum = lambda a, b: ld(a) + ld(b)
    return count


def spectrum_referee(lam):
    """count_ref from a spectrum known exactly: lam are exact numbers (ints, floats taken as exact, or mpmath.mpf)."""
    if mpmath is not None:
        lam = sorted(mpmath.mpf(x) for x in lam)

        def count(x):
            return bisect.bisect_right(lam, x)

        count.exact_sum = lambda a, b: mpmath.fadd(float(a), float(b), exact=True)
        return count
    lam = np.sort(np.asarray([np.longdouble(x) for x in lam]))

    def count(x):
        return int(np.searchsorted(lam, np.longdouble(x), side="right"))

    count.exact_sum = lambda a, b: np.longdouble(a) + np.longdouble(b)
    return count


# ------------------------------------------------------------------------------------------------ the checker
def tolerance(d, e, w, scale=1.0):
    """tol_j of the module docstring for the computed eigenvalues w of the matrix d, e (float64 array)."""
    p = prepare(d, e)
    w64 = np.abs(np.asarray(w).astype(np.float64))
    two_k = np.ldexp(1.0, p.k)
    stop = np.maximum(p.pivmin * two_k, 2.0 * EPS * w64)
    backward = C_BACKWARD * EPS * max(abs(p.gl), abs(p.gu)) * two_k
    rounding = (2.0 ** -24) * w64 if np.asarray(w).dtype == np.float32 else 0.0
    return scale * (stop + backward + rounding)


def check_eigenvalues(d, e, w, begin=0, count_ref=None, extra=0.0, scale=1.0):
    """None when every w[i], the computed eigenvalue begin + i of the matrix d, e, brackets the referee's eigenvalue
    within tol (+ extra, for a comparison value that carries an error of its own); else a description of the worst."""
    w = np.asarray(w)
    if not np.all(np.isfinite(w)):
        return f"not finite: {w[~np.isfinite(w)][:4]}"
    if count_ref is None:
        count_ref = sturm_referee(d, e)
    tol = tolerance(d, e, w, scale) + extra
    w64 = w.astype(np.float64)
    if hasattr(count_ref, "many"):
        below = count_ref.many(w64.astype(np.longdouble) - tol.astype(np.longdouble))
        above = count_ref.many(w64.astype(np.longdouble) + tol.astype(np.longdouble))
    else:
        below = np.array([count_ref(count_ref.exact_sum(x, -t)) for x, t in zip(w64, tol)], dtype=np.int64)
        above = np.array([count_ref(count_ref.exact_sum(x, t)) for x, t in zip(w64, tol)], dtype=np.int64)
    j = begin + np.arange(w.shape[0])
    badl = below > j
    badu = above < j + 1
    if badl.any() or badu.any():
        i = int(np.nonzero(badl | badu)[0][0])
        return (f"{int((badl | badu).sum())} of {w.shape[0]} eigenvalues outside their bracket; first: index {j[i]}, "
                f"w = {w64[i]!r}, tol = {tol[i]!r}, count_ref(w - tol) = {below[i]}, count_ref(w + tol) = {above[i]}")
    return None


def check_counts(counts, expected):
    """None when the counts equal the known integers exactly; else a description."""
    counts = np.asarray(counts)
    expected = np.asarray(expected)
    if counts.shape != expected.shape or not np.array_equal(counts, expected):
        i = np.nonzero(counts != expected)[0][:4] if counts.shape == expected.shape else []
        return f"counts differ at {list(i)}: {counts[i] if len(i) else counts.shape} != {expected[i] if len(i) else expected.shape}"
    return None


def diagonal_count_case(n, dtype):
    """An integer diagonal matrix (e = 0, zero pivots at its eigenvalues), shifts at the eigenvalues and the
    half-integers around them, and the exact counts."""
    rng = np.random.default_rng(1000 + n)
    d = rng.integers(-5, 6, size=n).astype(dtype)
    e = np.zeros(max(n - 1, 0), dtype=dtype)
    shifts = np.arange(-12, 13).astype(dtype) / 2        # -6, -5.5, ..., 6
    expected = np.array([(d <= s).sum() for s in shifts], dtype=np.int64)
    return d, e, shifts, expected


# ------------------------------------------------------------------------------------------------ matrices
def laplacian(n, dtype):
    d = np.full(n, 2.0, dtype=dtype)
    e = np.full(max(n - 1, 0), -1.0, dtype=dtype)
    return d, e


def laplacian_referee(n):
    """2 - 2 cos(j pi / (n + 1)), j = 1 .. n, to 160 bits (or long double)."""
    if mpmath is not None:
        with mpmath.workprec(160):
            lam = [2 - 2 * mpmath.cos(mpmath.pi * j / (n + 1)) for j in range(1, n + 1)]
        return spectrum_referee(lam)
    ld = np.longdouble
    return spectrum_referee(list(2 - 2 * np.cos(ld(np.pi) * np.arange(1, n + 1, dtype=ld) / (n + 1))))


def clement(n, dtype):
    """Clement / Kac matrix: zero diagonal, e_i = sqrt((i + 1)(n - 1 - i)); eigenvalues -(n-1), -(n-3), ..., n-1.  Its
    off-diagonal is irrational, so the matrix held in `dtype` is a perturbation of relative size eps(dtype) / 2 of
    Clement's: the referee is the Sturm count of the matrix as held (clement_spectrum is for the by-eye comparison)."""
    i = np.arange(n - 1, dtype=np.float64)
    return np.zeros(n, dtype=dtype), np.sqrt((i + 1) * (n - 1 - i)).astype(dtype)


def wilkinson(m, dtype, copies=1, glue=2.0 ** -30):
    """W_{2m+1}^+: d = |m - i|, e = 1; `copies` of it glued by a small off-diagonal entry."""
    d1 = np.abs(np.arange(-m, m + 1)).astype(dtype)
    e1 = np.ones(2 * m, dtype=dtype)
    d, e = d1, e1
    for _ in range(copies - 1):
        d = np.concatenate((d, d1))
        e = np.concatenate((e, np.asarray([glue], dtype=dtype), e1))
    return d, e


def with_splits(n, dtype):
    rng = np.random.default_rng(7)
    d = rng.standard_normal(n).astype(dtype)
    e = rng.standard_normal(n - 1).astype(dtype)
    e[[n // 5, n // 2, n // 2 + 1, n - 3]] = 0
    return d, e


def constant_diagonal(n, dtype, value=-3.75):
    return np.full(n, value, dtype=dtype), np.zeros(n - 1, dtype=dtype)


def graded(dtype, span=40):
    """entries from 2^-span to 2^span along the diagonal"""
    k = np.arange(-span, span + 1)
    d = np.ldexp(1.0 + 0.25 * np.cos(k), k).astype(dtype)
    e = np.ldexp(0.375, (k[:-1] + k[1:]) // 2).astype(dtype)
    return d, e


def random_tridiagonal(n, dtype, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(dtype), rng.standard_normal(n - 1).astype(dtype)


def model_matrices(dtype):
    """name -> (d, e, referee or None): small instances of the families the GPU test runs"""
    out = {
        "laplacian65": (*laplacian(65, dtype), laplacian_referee(65)),
        "clement40": (*clement(40, dtype), None),
        "wilkinson21": (*wilkinson(10, dtype), None),
        "wilkinson21x2": (*wilkinson(10, dtype, copies=2), None),
        "splits30": (*with_splits(30, dtype), None),
        "constant16": (*constant_diagonal(16, dtype), spectrum_referee([-3.75] * 16)),
        "graded": (*graded(dtype), None),
        "random130": (*random_tridiagonal(130, dtype), None),
        "random33_scaled": tuple(np.ldexp(x, 37).astype(dtype) for x in random_tridiagonal(33, dtype, 5)) + (None,),
        "one": (np.asarray([-2.5], dtype=dtype), np.zeros(0, dtype=dtype), spectrum_referee([-2.5])),
    }
    return out


# ------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["d", "s"])
def computed(request):
    """the model's eigenvalues of every matrix, once per type"""
    dtype = request.param
    mats = model_matrices(dtype)
    return dtype, {name: (d, e, ref if ref is not None else sturm_referee(d, e), eigenvalues(d, e))
                   for name, (d, e, ref) in mats.items()}


def test_model_passes_the_checker(computed):
    _, runs = computed
    for name, (d, e, ref, w) in runs.items():
        assert check_eigenvalues(d, e, w, count_ref=ref) is None, (name, check_eigenvalues(d, e, w, count_ref=ref))
        assert np.all(np.diff(w) >= 0), name


def test_observed_margin(computed):
    """Prints, per matrix, the smallest 2^-m by which tol can be scaled with the check still passing: the observed
    error against the derived bound.  The bound is not tuned to it (module docstring); the assertion is only that the
    unscaled bound holds."""
    dtype, runs = computed
    for name, (d, e, ref, w) in runs.items():
        m = 0
        while m < 12 and check_eigenvalues(d, e, w, count_ref=ref, scale=2.0 ** -(m + 1)) is None:
            m += 1
        print(f"{np.dtype(dtype).name} {name}: passes down to tol * 2^-{m}")
        assert check_eigenvalues(d, e, w, count_ref=ref) is None


def test_counts_are_exact_on_integer_diagonals():
    for dtype in (np.float64, np.float32):
        for n in (1, 2, 33):
            d, e, shifts, expected = diagonal_count_case(n, dtype)
            assert check_counts(sturm_count(d, e, shifts), expected) is None


def test_range_equals_slice_and_nan():
    d, e = random_tridiagonal(40, np.float64, 3)
    w = eigenvalues(d, e)
    assert np.array_equal(eigenvalues(d, e, 7, 19), w[7:19])
    assert eigenvalues(d, e, 5, 5).shape == (0,)
    d[3] = np.nan
    assert np.all(np.isnan(eigenvalues(d, e, 2, 9)))
    assert np.all(sturm_count(d, e, [0.0, 1.0]) == -1)


def test_power_of_two_scaling_is_exact():
    for dtype, j in ((np.float64, 300), (np.float64, -300), (np.float32, 40), (np.float32, -40)):
        d, e = random_tridiagonal(24, dtype, 9)
        w = eigenvalues(d, e)
        ws = eigenvalues(np.ldexp(d, j).astype(dtype), np.ldexp(e, j).astype(dtype))
        assert np.array_equal(ws, np.ldexp(w, j).astype(dtype))


def zero_pivot_matrix(dtype):
    """d = 0, e = 1 (n = 4): the Gershgorin interval is symmetric, so the first midpoint is exactly 0 and the first
    pivot there is an exact zero"""
    return np.zeros(4, dtype=dtype), np.ones(3, dtype=dtype)


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects_injected_faults(fault):
    dtype = np.float64
    if fault == "count_off_by_one":
        d, e, shifts, expected = diagonal_count_case(33, dtype)
        assert check_counts(sturm_count(d, e, shifts), expected) is None
        assert check_counts(sturm_count(d, e, shifts, fault=fault), expected) is not None
        return
    if fault == "no_pivmin_guard":
        d, e = zero_pivot_matrix(dtype)
    elif fault == "not_scaled_back":
        d, e = (np.ldexp(x, 37) for x in random_tridiagonal(33, dtype, 5))
    else:
        d, e = random_tridiagonal(130, dtype)
    ref = sturm_referee(d, e)
    assert check_eigenvalues(d, e, eigenvalues(d, e), count_ref=ref) is None
    assert check_eigenvalues(d, e, eigenvalues(d, e, fault=fault), count_ref=ref) is not None
