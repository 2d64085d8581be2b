"""The component-wise residual bound of tests/test_gpu_trsm_kernel.py applied to a whole triangular solve, on operands of
that test's "uniform" kind: diagonal entries of magnitude in [1, 2], the rest of the triangle uniform(-1, 1) / 8, the other
triangle -9.9.  A plain module: tests/test_gpu_solver.py (GPU) and tests/test_solver_cases.py (CPU half) import it.

Every side / uplo / op / diag is the row form X' T^H = B' of the kernel test:

    side R:  X op(A) = alpha B      X' = X      B' = alpha B        T = A (op C), conj(A) (op T), A^H (op N)
    side L:  op(A) X = alpha B      X' = X^H    B' = (alpha B)^H    T = op(A)

with T lower or upper triangular (diag U: a unit diagonal), swept from its first 64-block (lower) or its last (upper).
With R_j = B'_j - X'h_solved T_{j,solved}^H - X'h_j T_jj^H formed in the wide type from the result X'h, K_j the number of
columns solved before 64-block j ACROSS tiles (the block size of every shape is a multiple of 64, so the 64-blocks of the
tiles are the 64-blocks of the matrix), G_j = |B'_j| + |X'h_solved| |T_{j,solved}|^H, W_j the wide inverse of T_jj, u the
unit roundoff and c = 1 (real) or 4 (complex):

    |R_j| <= c (K_j + 67) u G_j (|W_j|^H |T_jj|^H),

the (K_j + 66) of the kernel test's derivation and one more rounding for alpha.  Where np.longdouble is no wider than
double the residual of d / z carries an error of its own and the factor is (2 K_j + 131), as there.  The bound of block j
depends only on B and on the blocks solved before it; no element is left out."""
import functools
import itertools

import numpy as np

from test_gpu_trsm_kernel import DT, JB, JUNK, WIDE, wide_inverse

SHAPES = [(260, 200, 64), (190, 321, 128)]
VARIANTS = list(itertools.product(SHAPES, "LR", "LU", "NTC", "NU"))


def alpha_of(t):
    return DT[t](complex(.7, -.4)) if t in "cz" else DT[t](.7)


@functools.lru_cache(maxsize=None)
def triangle(t, na, uplo, seed=23):
    """The stored triangular operand (Fortran order, read-only): the uplo triangle uniform, -9.9 in the other."""
    cx, dt = t in "cz", DT[t]
    rng = np.random.default_rng(seed + na)
    a = rng.uniform(-1, 1, (na, na)) / 8
    dg = rng.uniform(1, 2, na) * rng.choice([-1, 1], na)
    if cx:
        a = a + 1j * rng.uniform(-1, 1, (na, na)) / 8
        dg = dg * np.exp(2j * np.pi * rng.uniform(size=na))
    a[np.arange(na), np.arange(na)] = dg
    a[np.triu_indices(na, 1) if uplo == "L" else np.tril_indices(na, -1)] = JUNK
    a = np.asfortranarray(a.astype(dt))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rhs(t, m, n, seed=29):
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, (m, n)) + (1j * rng.uniform(-1, 1, (m, n)) if t in "cz" else 0)
    b = np.asfortranarray(b.astype(DT[t]))
    b.setflags(write=False)
    return b


def effective(a, side, uplo, op, diag):
    """(T, upper): the triangular matrix of the row form X' T^H = B' and whether it is upper triangular."""
    tri = np.tril(a) if uplo == "L" else np.triu(a)
    if diag == "U":
        d = np.arange(a.shape[0])
        tri[d, d] = 1
    if side == "R":
        t = {"C": tri, "T": np.conj(tri), "N": np.conj(tri).T}[op]
        flipped = op == "N"
    else:
        t = {"N": tri, "T": tri.T, "C": np.conj(tri).T}[op]
        flipped = op != "N"
    return np.ascontiguousarray(t), (uplo == "U") != flipped


def residual_ratio(t, side, uplo, op, diag, alpha, a, b, x):
    """(largest |R_j| / bound over every element, where it is): <= 1 for a correct solve."""
    cx, dt, hp = t in "cz", DT[t], WIDE[t]
    tri, upper = effective(a, side, uplo, op, diag)
    na = tri.shape[0]
    if not np.all(np.isfinite(x)):
        return float("inf"), "a result that is not finite"
    xw, bw = x.astype(hp), hp(alpha) * b.astype(hp)
    if side == "L":
        xw, bw = np.conj(xw).T, np.conj(bw).T
    tw = tri.astype(hp)
    abs_t, abs_x, abs_b = (np.abs(v).astype(np.float64) for v in (tri, xw, bw))
    u = np.finfo(dt).eps / 2
    wide = np.finfo(hp).eps < np.finfo(dt).eps
    worst, where = 0.0, ""
    for j in range(-(-na // JB)):
        cols = slice(j * JB, min(na, (j + 1) * JB))
        solved = slice(cols.stop, na) if upper else slice(0, cols.start)
        kj = solved.stop - solved.start
        r = bw[:, cols] - xw[:, solved] @ np.conj(tw[cols, solved]).T - xw[:, cols] @ np.conj(tw[cols, cols]).T
        g = abs_b[:, cols] + abs_x[:, solved] @ abs_t[cols, solved].T
        w = wide_inverse(tri[cols, cols], upper, hp)
        wl = np.abs(w).astype(np.float64).T @ abs_t[cols, cols].T
        factor = (kj + 67) if wide else (2 * kj + 131)
        ratio = np.abs(r).astype(np.float64) / ((4 if cx else 1) * factor * u * (g @ wl))
        if not ratio.max() <= worst:
            rr, cc = np.unravel_index(np.nanargmax(ratio), ratio.shape)
            worst, where = float(ratio.max()), f"row {rr} of X', 64-block {j} column {cc}"
    return worst, where


def drop_tile(a, uplo, nb):
    """A copy of the stored operand with its first off-diagonal nb x nb tile set to zero: the fault the bound must see."""
    out = a.copy(order="F")
    if uplo == "L":
        out[nb:2 * nb, :nb] = 0
    else:
        out[:nb, nb:2 * nb] = 0
    return out
