"""The tile POTRF kernels -- launch_potrf_coop (csrc/device/kernels_potrf_coop.hip, potrf_diag_core.hpp) and the chain
launch_potrf_diag + launch_trsm + launch_update per 64 columns -- called directly, one factorization of ONE kb x kb tile
per case, through dlaf.potrf_direct, against a plain numpy reference written from the contract in
csrc/device/device_api.hpp and not from the kernels:

    lower(tile[:kb, :kb]) <- L with A = L L^H (the diagonal of A taken as real; the diagonal of L positive with
    imaginary part exactly 0); winv block j <- inv(L_jj), 64 x 64 column-major, its strict upper triangle and every
    row and column past the block's extent exactly zero; nothing else of either buffer is read or written;
    a pivot that is not > 0 at column c: *info <- info_base + c + 1 (the first one wins), the 64-column blocks of L
    left of the failing one and their winv blocks are final; the cooperative launch fills the winv block of every
    strip that leaves early with NaN (*info != 0 on entry: all of them, tile untouched); the chain leaves them alone.

Buffers.  The tile buffer is flat, the tile at its start with leading dimension ld; the strict upper triangle holds NaN
(neither read nor written: a read that reaches arithmetic shows in the result), rows kb .. ld-1 and 64 elements behind
the tile hold a sentinel, complex inputs carry a non-zero imaginary part on the diagonal of A.  winv holds a sentinel
and one block more than the tile needs.  Everything outside lower(tile[:kb, :kb]) and the ceil(kb/64) blocks must come
back bit for bit (NaNs compared as bit patterns).  t_off / w_off place a buffer that many elements into its device
allocation: the entry fills what lies before it with a byte pattern and counts the bytes that no longer hold it after
the launches; the count must be 0.

Two kinds of operands, neither with a measured tolerance.

* exact.  Built backwards from L: each diagonal 64 x 64 block is D1 (I + N) D2, D1 and D2 diagonal powers of two in
  {1/2, 1, 2} and N the searched sparse strictly lower (Gaussian-)integer block of test_gpu_trsm_kernel.py whose inverse
  is a small integer matrix; the off-diagonal blocks are dense multiples of 2^-3 in [-1, 1]; A = L L^H in the wide type.
  Every pivot is a power of four, and every scaled column, every X_s = A(s,j) W_j^H, every partial sum of every Schur
  update in any order and every step of the inversion is exactly representable.  reference() asserts it: at each stage
  (A and the Schur sums; L_sj L_jj^H times W_j^H; the products L W and W (L W) of the inversion) the sum of the
  absolute values of the terms over their common power-of-two unit stays below 2^24 (s / c) or 2^53 (d / z); A must be
  representable; and a Cholesky factorization of A in the wide type must return the L the case was built from -- at
  every size for s / c (float64), up to kb = 321 for d / z, where the long double column loop is what would make the
  CPU half slow (at 512 and 1024 d / z hold the very numbers of s / c, which are factored there, and the same follows
  from uniqueness: A = L L^H holds exactly and L has a positive diagonal).
  s / c: sqrtf and the division are exact on these pivots, so L and every winv block must be EQUAL to the construction.
  d / z: the pivot path is pivot_sqrt, v_rsq_f64 plus coupled Newton steps.  test_pivot_sqrt_on_powers_of_four emulates
  its recurrence with exact fused multiply-adds for every pivot 4^k the cases use and seeds 2^-k (1 + delta), delta
  swept over [-2^-25, 2^-25]: sq == 2^k always, but inv == 2^-k only for |delta| < ~2^-27.3 -- the last correction of h
  is taken against an already exact g and only halves h's error, leaving inv up to 6 u off.  Whether the device is
  exact therefore hangs on the seed instruction, which the CPU cannot decide: the d / z exact cases are NOT asserted
  equal, they are judged by the bounds (i)-(iii) below.  Their residuals are formed without a wide type: with
  Delta = Lh - L and Omega = Wh - W (exact differences of neighbouring doubles), A - Lh Lh^H = -(L Delta^H + Delta L^H +
  Delta Delta^H) and Lh Wh - I = L Omega + Delta W + Delta Omega, evaluated in double with the evaluation's own
  gamma_{3 k} bound ADDED to the residual before it is compared -- which is what keeps kb = 512 and 1024 cheap.
  Every shape here, kb = 1024 included, fits in 24 bits (the largest load, A(s,j) W_j^H at kb = 1024, is below 2^18),
  so no exact case is restricted to d / z; test_exact_cases_fit prints the loads.

* uniform.  Off-diagonal entries uniform in (-1, 1) (+ i uniform(-1, 1)), A_ii = 1 + sum_{j != i} (|re| + |im|) +
  uniform(0, 1): by Gershgorin every eigenvalue, hence every pivot (a diagonal entry of a Schur complement), is >= 1;
  reference() checks the Gershgorin margin on the rounded matrix and the pivots of a double Cholesky.

Bounds.  u the unit roundoff, c = 1 (real) or 4 (complex multiply-adds written as real ones, as in the sibling tests),
|.| the modulus of a residual and |re| + |im| (`mag`) of an operand, gamma_k = k u / (1 - k u), Lh / Wh the device's
outputs, everything formed in the wide type (float64 for s / c, long double for d / z; where long double is no wider the
factors of d / z are doubled, the residual itself then carrying as much error again).  Block column by block column,
j = 0, 1, ..., each in the order (i), (ii), (iii), so that a bound never rests on something not yet checked:

(i)   diagonal block, lower triangle:
          |A_jj - sum_{k<=j} Lh_jk Lh_jk^H| <= c gamma_{64 j + 64 + p} (|A_jj| + sum_{k<=j} |Lh_jk| |Lh_jk|^H),  p = 17.
      Element (r, col), n = 64 j + col' columns left of it: whatever the order of the Schur sums and of the 16-column
      panels inside the block, sh = fl(a - sum_{k<n} l_rk conj(l_ck)) is n products and n subtractions:
      |sh - (a - sum)| <= gamma_{n+1} (|a| + sum |l||l|) (Higham, Accuracy and Stability, Lemma 8.4 / Thm 10.3; stores
      between steps do not round).  The pivot: sq = sqrt(dh)(1 + e1), inv = (1 + e2) / sqrt(dh).  pivot_sqrt states
      "within an ulp or two" (4 u) for a seed good to 2^-26; the sweep over seeds good to 2^-25 finds sq exact and
      inv within 6 u on powers of four, and the test keeps |e1|, |e2| <= 8 u, asserted on the CPU by the sweep test for powers of four and
      for random pivots.  sqrtf and the division of s / c are inside that.  l_rc = sh inv (1 + e3), |e3| <= u, so
      l_rc l_cc = sh (1 + theta), |theta| <= (8 + 8 + 1) u; on the diagonal l_cc^2 = dh (1 + e1)^2.  Hence
      |a - sum_{k<=n} l_rk conj(l_ck)| <= gamma_{n+1} (...) + 17 u |l_rc||l_cc| <= gamma_{n+1+17} (|a| + sum_{k<=n} |l||l|),
      n + 1 <= 64 j + 64.
(ii)  the inverse, as a RIGHT residual, D_j the block-diagonal matrix of the 16 x 16 products P_i = |L_ii| |Wh_ii|:
          |Lh_jj Wh_j - I| <= c gamma_q D_j (|Lh_jj| |Wh_j|),  q = 82.
      The inversion reads Lh_jj as stored, so the sums of the factorization enter through Lh_jj only and add no term.
      Diagonal 16-blocks are column-wise substitutions with at most 16 operations per entry:
      |L_ii Wh_ii - I| <= gamma_17 P_i (Higham Thm 8.5).  An off-diagonal 16-block (i > j) is Wh_ij = -fl(Wh_ii Th),
      Th = fl(sum_{j<=k<i} L_ik Wh_kj) = T + E1, |E1| <= gamma_48 S, S = sum |L_ik| |Wh_kj|, fl(Wh_ii Th) = Wh_ii Th + E2,
      |E2| <= gamma_16 |Wh_ii| |Th|.  Then (L Wh)_ij = T + L_ii Wh_ij = -E1 + (I - L_ii Wh_ii) Th - L_ii E2 and
      |(L Wh)_ij| <= gamma_48 S + (gamma_17 + gamma_16)(1 + gamma_48) P_i S.  diag(P_i) >= 1 - u (wh_kk = fl(1 / l_kk)), so
      S <= P_i S / (1 - u) and the whole is below gamma_82 P_i S (48 + 17 + 16 and one unit for the (1 - u) and the
      second-order terms); S <= (|L| |Wh|)_ij, and on the diagonal P_i <= P_i P_i / (1 - u).
(iii) each block (s, j) below it, G = |A_sj| + sum_{k<j} |Lh_sk| |Lh_jk|^H, F_j = |Lh_jj Wh_j - I| as measured in (ii):
          |A_sj - sum_{k<=j} Lh_sk Lh_jk^H| <= c [gamma_{64 j + 1} G + gamma_65 G |Wh_j|^H |Lh_jj|^H] + (1 + gamma_{64 j + 1}) G F_j^H.
      Ah = fl(A_sj - sum_{k<j} ...) = A_sj - sum + E1, |E1| <= gamma_{64 j + 1} G, |Ah| <= (1 + gamma) G;
      Xh = fl(Ah Wh_j^H) = Ah Wh_j^H + E2, |E2| <= gamma_64 |Ah| |Wh_j|^H.  The residual is
      (Ah - E1) - Xh Lh_jj^H = -E1 - Ah (Lh_jj Wh_j - I)^H - E2 Lh_jj^H: the derivation of test_gpu_trsm_kernel.py with the
      device's own Wh_j in place of a once-rounded inverse.
No element of the lower triangle is left out.

The CPU half (no GPU): a numpy emulation of the blocked right-looking algorithm in the working precision (per 64
columns: factor and invert the diagonal block, X = A W^H, the Schur update) goes through the same checker: equality on
every exact case, inside (i)-(iii) on every uniform case, and a FAILURE for each injected fault: one Schur block skipped,
one X block formed with W where W^H is meant, the imaginary part of one diagonal entry not dropped, one element of one
winv block one ulp off (exact class, s / c: one ulp lies inside the bounds d / z are judged by), one NaN of the upper
triangle overwritten, info off by one in a failing case."""
import decimal
import functools
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_trsm_kernel import BITS, DT, JB, LD_WIDER, TYPES, WIDE, bits_differ, int_block, mag, unit_of

gpu = pytest.mark.gpu

PATHS = ["coop", "chain"]
SENTINEL = {False: 1234.5, True: 1234.5 - 4321.25j}
W_SENTINEL = {False: -777.25, True: -777.25 + 55.5j}
TAIL = 64            # sentinel elements behind the tile
PB = 16              # inner panel of diag_factor_invert
P_PIVOT = 17         # (i): 8 u for sq, 8 u for inv, u for the scaling
Q_INVERSE = 82       # (ii): 48 + 17 + 16 + 1
PIVOT_ULPS = 8       # |e1|, |e2| <= 8 u, what P_PIVOT rests on and the sweep test asserts
D_Z_EQUALITY = False  # what the pivot_sqrt sweep decides (see the docstring): d / z exact cases are judged by the bounds

DEFAULTS = dict(ld=None, t_off=0, w_off=0, sync_zeroed_by=1, count_strips=1, info=0, info_base=0, bad=(), variant=None)


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


def resolve(spec):
    s = dict(DEFAULTS, **spec)
    s["ld"] = s["ld"] or s["kb"]
    return s


def nan_of(cx):
    return complex(np.nan, np.nan) if cx else np.nan


class Case:
    pass


def wide_cholesky(a, hp):
    """Lower Cholesky factor of the Hermitian matrix whose lower triangle is in `a`, column by column in the type hp."""
    n = a.shape[0]
    a = a.astype(hp)
    l = np.zeros((n, n), dtype=hp)
    for c in range(n):
        v = a[c:, c] - l[c:, :c] @ np.conj(l[c, :c])
        d = v[0].real
        assert d > 0
        l[c:, c] = v / np.sqrt(d)
        l[c, c] = np.sqrt(d)
    return l


@functools.lru_cache(maxsize=None)
def reference(t, kb, kind, bad=(), variant=None, seed=5):
    """The operands of one case and what the contract says comes out (cached and never modified: shared by the GPU
    tests and the CPU checks).  bad / variant: diagonal entries of A changed so that the pivot there is exactly 0
    ('zero'), -L_cc^2 ('negative') or NaN ('nan')."""
    cx = t in "cz"
    dt, hp = DT[t], WIDE[t]
    rng = np.random.default_rng(seed + 1000 * kb)
    nblk = -(-kb // JB)
    c = Case()
    c.t, c.kb, c.kind, c.nblk, c.bad, c.variant = t, kb, kind, nblk, tuple(bad), variant
    if kind == "exact":
        v = rng.integers(-8, 9, size=(kb, kb)) / 8
        if cx:
            v = v + 1j * (rng.integers(-8, 9, size=(kb, kb)) / 8)
        l = np.tril(v, -1).astype(dt)
        w = np.zeros((nblk, JB, JB), dtype=dt)
        for j in range(nblk):
            j0, jb = j * JB, min(JB, kb - j * JB)
            nn, mm = int_block(cx, j % 12)
            d1 = 2.0 ** rng.integers(-1, 2, size=JB)
            d2 = 2.0 ** rng.integers(-1, 2, size=JB)
            l[j0:j0 + jb, j0:j0 + jb] = (d1[:, None] * (np.eye(JB) + nn) * d2[None, :])[:jb, :jb]
            w[j, :jb, :jb] = ((1 / d2)[:, None] * mm * (1 / d1)[None, :])[:jb, :jb]
        dg = l[np.arange(kb), np.arange(kb)]
        assert np.all(dg.imag == 0) and np.all(dg.real > 0) and np.all(np.frexp(dg.real)[0] == 0.5)
        # A = L L^H: the double product is exact in any order once the sums below are shown to fit (53 bits at most),
        # which is what keeps kb = 1024 cheap; up to kb = 321 it is compared with the product in the wide type
        lw = l.astype(np.complex128 if cx else np.float64)
        a = lw @ np.conj(lw).T
        a_dt = a.astype(dt)
        # ---- every step exact in any order: sums of absolute values over the common unit
        bits = 2.0 ** BITS[t]
        ul, uw = unit_of(l), unit_of(w)
        ml = mag(l)
        c.exact_load = {"A and the Schur sums": 2 * (ml @ ml.T).max() / (ul * ul)}  # |A| + sum |L||L| <= 2 sum |L||L|
        for j in range(nblk):
            cols = slice(j * JB, min(kb, (j + 1) * JB))
            jb = cols.stop - cols.start
            ljj, wj = l[cols, cols], w[j][:jb, :jb]
            y = lw[cols.start:, cols] @ np.conj(lw[cols, cols]).T   # A(s, j) as the solve meets it, all s >= j
            p = mag(ljj) @ mag(wj)
            for what, v in (("A(s,j) W_j^H", (mag(y) @ mag(wj).T).max() / (ul * ul * uw)),
                            ("inversion L W", p.max() / (ul * uw)), ("inversion W (L W)", (mag(wj) @ p).max() / (uw * ul * uw))):
                c.exact_load[what] = max(c.exact_load.get(what, 0.0), float(v))
            assert np.array_equal(ljj.astype(np.complex128) @ wj.astype(np.complex128), np.eye(jb))
        c.fits = all(v < bits for v in c.exact_load.values())
        if c.fits:
            assert np.array_equal(a_dt.astype(a.dtype), a), "A is not representable"
            assert np.all(a_dt[np.arange(kb), np.arange(kb)].imag == 0)
        if (kb <= 321 or t in "sc") and c.fits:
            lh = l.astype(hp)
            assert np.array_equal(lh @ np.conj(lh).T, a.astype(hp)), "A formed in double differs from A formed in the wide type"
            assert np.array_equal(wide_cholesky(a, hp), lh), "the wide Cholesky does not return the L the case was built from"
        c.l, c.w = l, w
    else:
        assert not bad
        v = rng.uniform(-1, 1, size=(kb, kb))
        if cx:
            v = v + 1j * rng.uniform(-1, 1, size=(kb, kb))
        v = np.tril(v, -1)
        a_dt = (v + np.conj(v).T).astype(dt)
        a_dt[np.arange(kb), np.arange(kb)] = (1 + mag(a_dt).sum(axis=1) + rng.uniform(0, 1, size=kb)).astype(a_dt.real.dtype)
        a64 = a_dt.astype(np.complex128 if cx else np.float64)
        off = np.abs(a64).sum(axis=1) - np.abs(a64.diagonal())
        assert np.all(a64.diagonal().real - off >= 1), "Gershgorin: an eigenvalue may be below 1"
        assert np.all(np.linalg.cholesky(a64).diagonal().real ** 2 > 1), "a pivot is not above 1"
        assert np.array_equal(a_dt, np.conj(a_dt).T)
        c.l = c.w = None
        c.fits = True
    a_dt = a_dt.copy()
    for col in bad:
        lcc2 = (c.l[col, col].real ** 2).astype(a_dt.real.dtype)
        a_dt[col, col] = {"zero": a_dt[col, col].real - lcc2, "negative": a_dt[col, col].real - 2 * lcc2, "nan": np.nan}[variant]
    c.a = a_dt
    return c


def buffers(c, s):
    """(tile buffer, winv buffer, mask of the lower triangle) as a launch is given them."""
    cx, dt, kb, ld = c.t in "cz", DT[c.t], c.kb, s["ld"]
    t0 = np.full(ld * kb + TAIL, SENTINEL[cx], dtype=dt)
    view = t0[:ld * kb].reshape(kb, ld).T[:kb, :]
    low = np.tril(np.ones((kb, kb), dtype=bool))
    a = c.a.copy()
    if cx:  # the diagonal is taken as real: what its imaginary part holds must not matter
        a[np.arange(kb), np.arange(kb)] += 1j * (0.375 + (np.arange(kb) % 5))
    view[:] = np.where(low, a, nan_of(cx))
    mask = np.zeros(t0.size, dtype=bool)
    mask[:ld * kb].reshape(kb, ld).T[:kb, :] = low
    w0 = np.full((c.nblk + 1) * JB * JB, W_SENTINEL[cx], dtype=dt)
    return t0, w0, mask


def gamma(k, u):
    assert k * u < 0.5
    return k * u / (1 - k * u)


def check(c, s, path, got_t, got_w, info_out, t0, w0, mask, before_changed=0):
    """The one checker: the GPU's result and the emulation's go through it.  Returns the largest residual / bound of
    (i)-(iii), or 0.0 where nothing but equality was checked."""
    t, kb, nblk, ld = c.t, c.kb, c.nblk, s["ld"]
    cx, dt, hp = t in "cz", DT[t], WIDE[t]
    assert before_changed == 0, f"{before_changed} bytes in front of the tile or the winv buffer changed"
    outside = np.flatnonzero(bits_differ(got_t, t0) & ~mask)
    assert outside.size == 0, (f"{outside.size} elements outside the lower triangle changed; first: flat index {outside[0]} "
                               f"(row {outside[0] % ld}, column {outside[0] // ld}): {t0[outside[0]]} -> {got_t[outside[0]]}")
    assert not bits_differ(got_w[nblk * JB * JB:], w0[nblk * JB * JB:]).any(), "winv past the last block changed"
    wb = got_w[:nblk * JB * JB].reshape(nblk, JB, JB).transpose(0, 2, 1)  # [block][row][col]
    all_nan = lambda blk: bool(np.all(np.isnan(blk.real)) and (not cx or np.all(np.isnan(blk.imag))))
    if s["info"] != 0:
        assert info_out == s["info"], f"*info = {s['info']} on entry came back as {info_out}"
        assert not bits_differ(got_t, t0).any(), "the tile changed although *info != 0"
        if path == "coop":
            assert all(all_nan(wb[j]) for j in range(nblk)), "coop, *info != 0: a winv block is not NaN in every element"
        else:
            assert not bits_differ(got_w, w0).any(), "chain: winv changed although *info != 0"
        return 0.0
    if c.bad:
        col = min(c.bad)
        assert info_out == s["info_base"] + col + 1, f"info = {info_out}, expected {s['info_base']} + {col} + 1"
        jf = col // JB
        if path == "coop":
            for j in range(jf, nblk):
                assert all_nan(wb[j]), f"coop: winv block {j} (failing strip {jf}) is not NaN in every element"
        else:
            assert not bits_differ(got_w[jf * JB * JB:], w0[jf * JB * JB:]).any(), \
                f"chain: a winv block from the failing one ({jf}) on changed"
    else:
        assert info_out == 0, f"info = {info_out} on a positive definite tile"
        jf = nblk
    nf = min(kb, jf * JB)  # columns that are final
    lh = np.where(np.tril(np.ones((kb, kb), dtype=bool)), got_t[:ld * kb].reshape(kb, ld).T[:kb, :], 0)
    for j in range(jf):
        jb = min(JB, kb - j * JB)
        z = wb[j].copy()
        z[:jb, :jb][np.tril(np.ones((jb, jb), dtype=bool))] = 0
        assert np.all(z == 0), f"winv block {j}: an element of the strict upper triangle or past row / column {jb} is not zero"
    if cx:
        dgi = lh[np.arange(nf), np.arange(nf)].imag
        assert np.all(dgi == 0), f"diagonal of L, column {int(np.flatnonzero(dgi != 0)[0])}: imaginary part not 0"
    if c.kind == "exact" and (t in "sc" or D_Z_EQUALITY):
        badl = np.argwhere(np.tril(lh != c.l)[:, :nf])
        assert badl.size == 0, (f"{len(badl)} elements of L differ; first: ({badl[0][0]},{badl[0][1]}) strip {badl[0][0] // JB} block "
                                f"column {badl[0][1] // JB}: got {lh[tuple(badl[0])]}, expected {c.l[tuple(badl[0])]}")
        badw = np.argwhere(wb[:jf] != c.w[:jf])
        assert badw.size == 0, (f"{len(badw)} elements of winv differ; first: block {badw[0][0]} ({badw[0][1]},{badw[0][2]}): got "
                                f"{wb[tuple(badw[0])]}, expected {c.w[tuple(badw[0])]}")
        return 0.0
    # ---- (i)-(iii), block column by block column
    assert np.all(np.isfinite(lh[:, :nf])), "L is not finite"
    u = np.finfo(dt).eps / 2
    cc = 4 if cx else 1
    perturb = c.kind == "exact"  # d / z: residuals from the exact differences, evaluated in double
    dbl = 1 if (perturb or np.finfo(hp).eps < np.finfo(dt).eps) else 2
    f64 = np.complex128 if cx else np.float64
    u64 = np.finfo(np.float64).eps / 2
    mlh = mag(lh)
    if perturb:
        lx = c.l.astype(f64)
        dl = lh.astype(f64) - lx
        mlx, mdl = mag(lx), mag(dl)
    else:
        lhw, aw = lh.astype(hp), c.a.astype(hp)
    ma = mag(np.where(np.eye(kb, dtype=bool), c.a.real, c.a))
    worst = 0.0

    def judge(what, j, r, bound, r0=0, c0=0, tri=False):
        nonlocal worst
        r = np.asarray(r, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(r == 0, 0.0, r / bound)  # (an exact zero needs no bound; NaN and r > bound = 0 fail)
        if tri:
            ratio = np.tril(ratio)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        if not ratio.max() <= 1.0:
            rr, k = np.unravel_index(np.argmax(ratio), ratio.shape)
            pytest.fail(f"({what}) block column {j}, element ({r0 + rr},{c0 + k}) (strip {(r0 + rr) // JB}): |residual| = "
                        f"{float(r[rr, k]):.3e} is {ratio[rr, k]:.2f} x the bound {bound[rr, k]:.3e}")
        worst = max(worst, float(ratio.max()))

    for j in range(jf):
        c0, c1 = j * JB, min(kb, (j + 1) * JB)
        jb = c1 - c0
        # the residual of the whole block column, rows c0 .. kb, and its evaluation error
        if perturb:
            r = -(lx[c0:, :c1] @ np.conj(dl[c0:c1, :c1]).T + dl[c0:, :c1] @ np.conj(lx[c0:c1, :c1]).T +
                  dl[c0:, :c1] @ np.conj(dl[c0:c1, :c1]).T)
            ev = cc * gamma(3 * c1 + 2, u64) * (mlx[c0:, :c1] @ mdl[c0:c1, :c1].T + mdl[c0:, :c1] @ mlx[c0:c1, :c1].T +
                                                 mdl[c0:, :c1] @ mdl[c0:c1, :c1].T)
            r = np.abs(r) + ev
        else:
            a_col = aw[c0:, c0:c1].copy()
            a_col[np.arange(jb), np.arange(jb)] = a_col[np.arange(jb), np.arange(jb)].real
            r = np.abs(a_col - lhw[c0:, :c1] @ np.conj(lhw[c0:c1, :c1]).T).astype(np.float64)
        g = ma[c0:, c0:c1] + mlh[c0:, :c0] @ mlh[c0:c1, :c0].T
        ljj, wj = lh[c0:c1, c0:c1], wb[j][:jb, :jb]
        mljj, mwj = mlh[c0:c1, c0:c1], mag(wj)
        # (i)
        judge("i", j, r[:jb], cc * dbl * gamma(JB * j + JB + P_PIVOT, u) * (g[:jb] + mljj @ mljj.T), c0, c0, tri=True)
        # (ii)
        assert np.all(np.isfinite(wj)), f"winv block {j} is not finite"
        if perturb:
            wx = c.w[j][:jb, :jb].astype(f64)
            om = wj.astype(f64) - wx
            ljx, djx = lx[c0:c1, c0:c1], dl[c0:c1, c0:c1]
            f = np.abs(ljx @ om + djx @ wx + djx @ om) + cc * gamma(3 * jb + 2, u64) * (
                mag(ljx) @ mag(om) + mag(djx) @ mag(wx) + mag(djx) @ mag(om))
        else:
            f = np.abs(ljj.astype(hp) @ wj.astype(hp) - np.eye(jb, dtype=hp)).astype(np.float64)
        dj = np.zeros((jb, jb))
        for i0 in range(0, jb, PB):
            i1 = min(jb, i0 + PB)
            dj[i0:i1, i0:i1] = mljj[i0:i1, i0:i1] @ mwj[i0:i1, i0:i1]
        judge("ii", j, f, cc * dbl * gamma(Q_INVERSE, u) * (dj @ (mljj @ mwj)) + np.triu(np.full((jb, jb), np.inf), 1), c0, c0)
        assert np.all(f[np.triu_indices(jb, 1)] == 0), f"(ii) block {j}: the residual above the diagonal is not zero"
        # (iii)
        if c1 < kb:
            gl = g[jb:]
            bound = cc * dbl * (gamma(JB * j + 1, u) * gl + gamma(65, u) * (gl @ (mwj.T @ mljj.T))) + \
                (1 + gamma(JB * j + 1, u)) * (gl @ f.T)
            judge("iii", j, r[jb:], bound, c1, c0)
    return worst


def run_case(dlaf, t, spec, kind, path):
    s = resolve(spec)
    c = reference(t, s["kb"], kind, tuple(s["bad"]), s["variant"])
    assert c.fits, f"the exact case does not fit in {BITS[t]} bits: {c.exact_load}"
    t0, w0, mask = buffers(c, s)
    got_t, got_w = t0.copy(), w0.copy()
    info, before_changed = dlaf.potrf_direct(got_t, got_w, path=path, offsets=(s["t_off"], s["w_off"]),
                             **{k: s[k] for k in ("kb", "ld", "info", "info_base", "sync_zeroed_by", "count_strips")})
    worst = check(c, s, path, got_t, got_w, info, t0, w0, mask, before_changed)
    print(f"{path} {kind} {t} {spec}: max |residual| / bound = {worst:.3f}")
    return worst


# ---- the emulation ---------------------------------------------------------------------------------------------------
def emulate(c, s, path, fault=None):
    """The blocked right-looking algorithm in the working precision.  Returns (tile buffer, winv buffer, info) as a
    launch would leave them.  fault: None, 'skip', 'w-not-wh', 'imag', 'ulp', 'upper' or 'info'."""
    t, kb, nblk, ld = c.t, c.kb, c.nblk, s["ld"]
    cx, dt = t in "cz", DT[t]
    rdt = np.dtype(dt).type(0).real.dtype.type
    t0, w0, _ = buffers(c, s)
    got_t, got_w = t0.copy(), w0.copy()
    if s["info"] != 0:
        if path == "coop":
            got_w[:nblk * JB * JB] = nan_of(cx)
        return got_t, got_w, s["info"]
    view = got_t[:ld * kb].reshape(kb, ld).T[:kb, :]
    a = np.tril(view).astype(dt)
    a[np.arange(kb), np.arange(kb)] = a[np.arange(kb), np.arange(kb)].real
    wb = got_w[:nblk * JB * JB].reshape(nblk, JB, JB)
    info = 0
    jfault = max(0, nblk - 2)  # the block column a fault goes into
    for j in range(nblk):
        c0, c1 = j * JB, min(kb, (j + 1) * JB)
        jb = c1 - c0
        l = a[c0:c1, c0:c1].copy()
        for k in range(jb):
            d = l[k, k].real
            if not d > 0:
                info = s["info_base"] + c0 + k + 1
                break
            sq = np.sqrt(rdt(d))
            l[k, k] = sq
            l[k + 1:, k] = l[k + 1:, k] * (rdt(1) / sq)
            upd = l[k + 1:, k + 1:] - np.outer(l[k + 1:, k], np.conj(l[k + 1:, k]))
            l[k + 1:, k + 1:] = upd
            if cx:
                l[np.arange(k + 1, jb), np.arange(k + 1, jb)] = l[np.arange(k + 1, jb), np.arange(k + 1, jb)].real
        if info:
            if path == "coop":
                wb[j:] = nan_of(cx)
            break
        l = np.tril(l)
        w = np.zeros((jb, jb), dtype=dt)
        for i in range(jb):
            e = np.zeros(jb, dtype=dt)
            e[i] = 1
            w[i, :] = (e - l[i, :i] @ w[:i, :]) / l[i, i].real
        w = np.tril(w)
        if fault == "ulp" and j == jfault:
            v = w[jb // 2, 0] if jb > 1 else w[0, 0]
            w[jb // 2 if jb > 1 else 0, 0] = np.nextafter(rdt(v.real), rdt(np.inf)) + (1j * v.imag if cx else 0)
        a[c0:c1, c0:c1] = l
        blk = np.zeros((JB, JB), dtype=dt)
        blk[:jb, :jb] = w
        wb[j] = blk.T
        if c1 < kb:
            x = a[c1:, c0:c1] @ (w if (fault == "w-not-wh" and j == jfault) else np.conj(w).T)
            assert x.dtype == dt
            a[c1:, c0:c1] = x
            for sb in range(j + 1, nblk):
                for cb in range(j + 1, sb + 1):
                    if fault == "skip" and j == jfault and sb == nblk - 1 and cb == nblk - 1:
                        continue
                    rs, cs = slice(sb * JB, min(kb, sb * JB + JB)), slice(cb * JB, min(kb, cb * JB + JB))
                    a[rs, cs] = a[rs, cs] - a[rs, c0:c1] @ np.conj(a[cs, c0:c1]).T
            if cx:
                a[np.arange(c1, kb), np.arange(c1, kb)] = a[np.arange(c1, kb), np.arange(c1, kb)].real
    low = np.tril(np.ones((kb, kb), dtype=bool))
    view[low] = a[low]
    if fault == "imag":
        k = min(kb - 1, jfault * JB + 3)
        view[k, k] = view[k, k].real + 1j * t0[:ld * kb].reshape(kb, ld).T[k, k].imag
    if fault == "upper":
        view[0, kb - 1] = 0
    if fault == "info":
        info += 1
    return got_t, got_w, info


# ---- the cases -------------------------------------------------------------------------------------------------------
# kb        why
# 1..64     one strip: the inner 16-column panel boundary of diag_factor_invert, the identity tail beyond jb
# 65        two strips, the second one row (rows_s = 1 in every predicate); 100, 128, 129
# 192, 200  three strips: the first coop_wait_all with a non-empty set
# 256, 321  four and six strips: s >= 3 runs the real-type X prefetch (cc + 1 < s) and the non-to_lds diagonal update;
#           at 321 the last strip has one row
# 512       the workload's nb, eight strips: exact class only
# 1024      sixteen strips: exact class only (its sums fit in 24 bits too, so s / c run it as well as d / z)
SIZES = (1, 15, 16, 17, 63, 64, 65, 100, 128, 129, 192, 200, 256, 321)
EXACT_CASES = [(t, kb) for kb in SIZES + (512, 1024) for t in TYPES]
UNIFORM_CASES = [(t, kb) for kb in SIZES for t in TYPES]
PLACEMENT = {
    "ld=kb+3": dict(kb=200, ld=203),
    "ld=4104 window of a tall array": dict(kb=200, ld=4104),
    "t_off=1": dict(kb=200, t_off=1),
    "t_off=1 ld=kb+3": dict(kb=200, ld=203, t_off=1),
    "w_off=4": dict(kb=200, w_off=4),
    "info_base=3584": dict(kb=200, info_base=7 * 512),
}
SYNC = {f"sync_zeroed_by={z} count_strips={n}": dict(kb=200, sync_zeroed_by=z, count_strips=n, ld=208)
        for z in (0, 1) for n in (0, 1)}
INFO_SET = {"info=5 on entry": dict(kb=200, info=5, ld=203), "info=-7 on entry": dict(kb=200, info=-7, info_base=3584)}
BAD_COLS = (0, 15, 16, 63, 64, 127, 128, 199)
NOT_SPD = {f"zero pivot at {col}": dict(kb=200, bad=(col,), variant="zero") for col in BAD_COLS}
NOT_SPD.update({f"negative pivot at {col}": dict(kb=200, bad=(col,), variant="negative") for col in BAD_COLS})
NOT_SPD.update({f"NaN pivot at {col}": dict(kb=200, bad=(col,), variant="nan") for col in BAD_COLS})
NOT_SPD["zero pivots at 70 and 140"] = dict(kb=200, bad=(70, 140), variant="zero")


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t,kb", [pytest.param(t, kb, id=f"kb={kb}, {t}") for t, kb in EXACT_CASES])
def test_potrf_exact(dlaf, t, kb, path):
    run_case(dlaf, t, dict(kb=kb), "exact", path)


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t,kb", [pytest.param(t, kb, id=f"kb={kb}, {t}") for t, kb in UNIFORM_CASES])
def test_potrf_uniform_componentwise_bounds(dlaf, t, kb, path):
    run_case(dlaf, t, dict(kb=kb), "uniform", path)


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", list(PLACEMENT))
def test_potrf_leading_dimension_and_placement(dlaf, name, t, path):
    run_case(dlaf, t, PLACEMENT[name], "exact", path)
    run_case(dlaf, t, PLACEMENT[name], "uniform", path)


@gpu
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", list(SYNC))
def test_potrf_coop_sync_and_strip_count(dlaf, name, t):
    """red2band's combination (the launcher zeroes sync, no strip count) and the factorization's, and the two between."""
    run_case(dlaf, t, SYNC[name], "exact", "coop")
    run_case(dlaf, t, SYNC[name], "uniform", "coop")


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", list(INFO_SET))
def test_potrf_info_set_on_entry(dlaf, name, t, path):
    run_case(dlaf, t, INFO_SET[name], "exact", path)


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("name", list(NOT_SPD))
def test_potrf_not_positive_definite(dlaf, name, t, path):
    for info_base in (0, 7 * 512):
        run_case(dlaf, t, dict(NOT_SPD[name], info_base=info_base, ld=203 if info_base else 200), "exact", path)


@gpu
def test_potrf_direct_refuses_out_of_bounds(dlaf):
    """The entry launches nothing when a field would make a kernel touch memory outside a buffer."""
    c = reference("d", 200, "exact")
    s = resolve(dict(kb=200, ld=203))
    t0, w0, _ = buffers(c, s)
    base = dict(kb=200, ld=203, info=0, info_base=0, sync_zeroed_by=1, count_strips=1)
    for path in PATHS:
        for change in (dict(kb=201), dict(kb=0), dict(ld=199), dict(ld=204), dict(sync_zeroed_by=2)):
            tb, wbuf = t0.copy(), w0.copy()
            with pytest.raises(ValueError):
                dlaf.potrf_direct(tb, wbuf, path=path, **dict(base, **change))
            assert not bits_differ(tb, t0).any() and not bits_differ(wbuf, w0).any()
        with pytest.raises(ValueError):
            dlaf.potrf_direct(t0.copy(), w0[:3 * JB * JB].copy(), path=path, **base)   # winv too short
        with pytest.raises(ValueError):
            dlaf.potrf_direct(t0.copy(), w0.copy(), path=path, offsets=(0, 1), **base)  # winv off 16-byte alignment


# ---- the CPU half ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_exact_cases_fit(t):
    """No GPU: the exactness assertions of reference() for every exact case of one type; prints the largest loads."""
    for tt, kb in EXACT_CASES:
        if tt == t:
            c = reference(t, kb, "exact")
            assert c.fits, (t, kb, c.exact_load)
    for spec in NOT_SPD.values():
        assert reference(t, spec["kb"], "exact", tuple(spec["bad"]), spec["variant"]).fits
    print(f"kb = 1024, {t}: {reference(t, 1024, 'exact').exact_load}")


def exact_fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding: a correctly rounded fused multiply-add


def pivot_sqrt_emulated(d, r):
    """pivot_sqrt of potrf_diag_core.hpp on the seed r ~ 1 / sqrt(d)."""
    g, h = d * r, 0.5 * r
    e = exact_fma(-h, g, 0.5)
    g, h = exact_fma(g, e, g), exact_fma(h, e, h)
    e = exact_fma(-g, g, d)
    g = exact_fma(e, h, g)
    e = exact_fma(-h, g, 0.5)
    h = exact_fma(h, e, h)
    e = exact_fma(-g, g, d)
    return exact_fma(e, h, g), h + h


def test_pivot_sqrt_on_powers_of_four():
    """No GPU: decides whether d / z may be asserted EQUAL (D_Z_EQUALITY) and backs the constant P_PIVOT.  The
    recurrence of pivot_sqrt with exact fused multiply-adds on every pivot 4^k the exact cases have (the diagonal of L
    is a product of two entries of {1/2, 1, 2}) from seeds 2^-k (1 + delta), delta dense in [-2^-25, 2^-25], and on
    random pivots against a 50-digit square root."""
    u = 2.0 ** -53
    ks = sorted({int(np.log2(v)) for t, kb in EXACT_CASES for v in reference(t, kb, "exact").l.diagonal().real})
    assert ks == [-2, -1, 0, 1, 2]
    deltas = np.concatenate([np.linspace(-2.0 ** -25, 2.0 ** -25, 1501), [0.0, -2.0 ** -26, 2.0 ** -26]])
    sq_exact = inv_exact = True
    worst_sq = worst_inv = 0.0
    for k in ks:
        for delta in deltas:
            sq, inv = pivot_sqrt_emulated(4.0 ** k, 2.0 ** -k * (1 + delta))
            sq_exact &= sq == 2.0 ** k
            inv_exact &= inv == 2.0 ** -k
            worst_sq, worst_inv = max(worst_sq, abs(sq * 2.0 ** -k - 1) / u), max(worst_inv, abs(inv * 2.0 ** k - 1) / u)
    print(f"powers of four: sq exact: {sq_exact}, inv exact: {inv_exact}; worst errors {worst_sq:.2f} u, {worst_inv:.2f} u")
    assert sq_exact
    assert inv_exact == D_Z_EQUALITY, "pivot_sqrt changed: revisit D_Z_EQUALITY (and the docstring)"
    assert worst_inv <= PIVOT_ULPS
    # the seed the recurrence is exact from (documentation of the margin; the device's seed is not known here)
    assert pivot_sqrt_emulated(1.0, 1 + 2.0 ** -28) == (1.0, 1.0) and pivot_sqrt_emulated(1.0, 1 - 2.0 ** -28) == (1.0, 1.0)
    rng = np.random.default_rng(3)
    decimal.getcontext().prec = 50
    for d, delta in zip(rng.uniform(1, 4, size=600) * 2.0 ** rng.integers(-8, 9, size=600) * 1.0,
                        rng.uniform(-2.0 ** -25, 2.0 ** -25, size=600)):
        root = decimal.Decimal(float(d)).sqrt()
        sq, inv = pivot_sqrt_emulated(float(d), float(1 / root) * (1 + delta))
        assert abs(decimal.Decimal(sq) / root - 1) <= PIVOT_ULPS * decimal.Decimal(u)
        assert abs(decimal.Decimal(inv) * root - 1) <= PIVOT_ULPS * decimal.Decimal(u)


def all_specs():
    """(t, spec, kind) of every GPU case."""
    out = [(t, dict(kb=kb), "exact") for t, kb in EXACT_CASES] + [(t, dict(kb=kb), "uniform") for t, kb in UNIFORM_CASES]
    for t in TYPES:
        out += [(t, sp, kind) for sp in list(PLACEMENT.values()) + list(SYNC.values()) for kind in ("exact", "uniform")]
        out += [(t, sp, "exact") for sp in INFO_SET.values()]
        out += [(t, dict(sp, info_base=info_base, ld=203 if info_base else 200), "exact") for sp in NOT_SPD.values()
                for info_base in (0, 7 * 512)]
    return out


def checked_emulation(t, spec, kind, path, fault=None):
    s = resolve(spec)
    c = reference(t, s["kb"], kind, tuple(s["bad"]), s["variant"])
    t0, w0, mask = buffers(c, s)
    got_t, got_w, info = emulate(c, s, path, fault)
    return check(c, s, path, got_t, got_w, info, t0, w0, mask)


@pytest.mark.parametrize("t", TYPES)
def test_emulation_passes_every_case(t):
    """No GPU.  The working-precision emulation through the checker the GPU results go through, one type per test:
    equality on every exact case (the bounds for d / z), inside (i)-(iii) on every uniform case."""
    worst = 0.0
    for tt, spec, kind in all_specs():
        if tt != t:
            continue
        for path in PATHS:
            if path == "chain" and not (spec.get("bad") or spec.get("info")):
                continue  # the emulation differs between the paths in what an early exit leaves only
            worst = max(worst, checked_emulation(t, spec, kind, path))
    print(f"emulation: max |residual| / bound = {worst:.3f}")
    assert 0 < worst <= 1


FAULT_TARGETS = [(t, dict(kb=kb, ld=kb + 3), kind) for t in TYPES for kb in (200, 321) for kind in ("exact", "uniform")]


@pytest.mark.parametrize("fault", ["skip", "w-not-wh", "imag", "ulp", "upper", "info"])
def test_injected_fault_is_detected(fault):
    """No GPU: every injected fault must make the checker fail."""
    n = 0
    for t, spec, kind in FAULT_TARGETS:
        if fault == "imag" and t not in "cz":
            continue
        if fault == "ulp" and not (kind == "exact" and (t in "sc" or D_Z_EQUALITY)):
            continue
        if fault == "info":
            if kind != "exact" or spec["kb"] != 200:
                continue
            spec = dict(spec, bad=(127,), variant="zero", info_base=7 * 512)
        for path in PATHS:
            with pytest.raises(BaseException) as e:
                checked_emulation(t, spec, kind, path, fault)
            assert isinstance(e.value, (AssertionError, pytest.fail.Exception)), (t, spec, kind, fault, e.value)
            n += 1
    assert n >= 4


def test_changed_surroundings_are_detected():
    """No GPU: a byte in front of a buffer, and on the chain a winv block from the failing one on, must not change."""
    spec = dict(kb=200, bad=(70,), variant="zero", info_base=7 * 512, ld=203)
    s = resolve(spec)
    c = reference("d", 200, "exact", (70,), "zero")
    t0, w0, mask = buffers(c, s)
    got_t, got_w, info = emulate(c, s, "chain")
    check(c, s, "chain", got_t, got_w, info, t0, w0, mask)
    with pytest.raises(AssertionError):
        check(c, s, "chain", got_t, got_w, info, t0, w0, mask, before_changed=8)
    got_w[2 * JB * JB + 5] = 0
    with pytest.raises(AssertionError):
        check(c, s, "chain", got_t, got_w, info, t0, w0, mask)
