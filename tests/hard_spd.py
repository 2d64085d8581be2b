"""Inputs, references and checkers of test_hard_spd.py (CPU) and test_gpu_cholesky_hard.py (GPU): Hermitian positive
definite matrices that are NOT diagonally dominant, matrices that are not positive definite in a decisive way, and the
measures the Cholesky drivers are held to on them.  Nothing here touches the GPU.

Every input is cached, built in float64 / complex128, rounded once to the working type and made exactly Hermitian again;
what the device sees is that rounded matrix, and every reference is computed from it.  The wide type (float64 /
complex128 for s / c, longdouble / clongdouble for d / z where longdouble is wider) follows test_gpu_trsm_kernel.py.

Calibrated reference ratios (calibrate(): scipy 1.15.3 / OpenBLAS ?potrf and cho_solve in the working precision on the
same rounded inputs, x86-64; worst value over the whole input set, both uplo) and the bars, 4 x the reference:

                         s        c        d        z
    factor, normwise     0.01317  0.01824  0.01623  0.01795     bars  0.05268  0.07296  0.06492  0.07180
    factor, componentw.  0.04460  0.05080  0.05634  0.04997     bars  0.17840  0.20320  0.22536  0.19988
    solve, backward         -        -     0.01004  0.008721    bars     -        -     0.04016  0.034884

(every worst case is at n = 129; the ratios fall with n).  test_hard_spd.py measures them again and holds these records
to within a factor of two of what it measures.
"""
import functools

import numpy as np
import scipy.linalg as sl

DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
LD_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
WIDE = {"s": np.float64, "c": np.complex128,
        "d": np.longdouble if LD_WIDER else np.float64, "z": np.clongdouble if LD_WIDER else np.complex128}
JB = 64  # columns of one inverted diagonal block
PAD = 3
SENTINEL = -9.9

FAMILIES = ["geo", "one_large", "one_small", "graded"]
SIZES = [(129, 64), (300, 100), (515, 128), (1024, 256)]
SOLVE_SIZES = [(515, 128), (129, 64)]
SOLVE_FAMILIES = ["geo", "one_small"]
NRHS = [7, 130]

# worst ratio of the working-precision LAPACK route over the whole input set: [normwise, componentwise] / backward
REF_FACTOR = {"s": [0.01317, 0.04460], "c": [0.01824, 0.05080], "d": [0.01623, 0.05634], "z": [0.01795, 0.04997]}
REF_SOLVE = {"d": 0.01004, "z": 0.008721}
BAR_FACTOR = {t: [4 * r for r in v] for t, v in REF_FACTOR.items()}
BAR_SOLVE = {t: 4 * r for t, r in REF_SOLVE.items()}


def eps_of(t):
    return float(np.finfo(DT[t]).eps)


def sizes_of(t):
    return SIZES[:3] if t == "z" else SIZES


def kappa_of(name, t):
    if name == "graded":
        return 1e3 if t in "dz" else 1e2
    return 1e10 if t in "dz" else 1e3


def grading_of(t):
    """exponent range of the two-sided scaling of `graded`"""
    return -8.0 if t in "dz" else -3.0


def frozen(a):
    a.setflags(write=False)
    return a


def hermitian_rounded(a, t):
    """`a` rounded once to the working type and made exactly Hermitian (the lower triangle decides, real diagonal)"""
    r = np.asarray(a).astype(DT[t])
    low = np.tril(r, -1)
    return np.asfortranarray(low + low.conj().T + np.diag(np.diagonal(r).real).astype(DT[t]))


@functools.lru_cache(maxsize=None)
def unitary(t, n, seed):
    """the Q of a QR of a seeded Gaussian matrix (complex for c / z), float64 / complex128"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, n))
    if t in "cz":
        g = g + 1j * rng.standard_normal((n, n))
    return frozen(np.linalg.qr(g)[0])


def spectrum_of(name, t, n):
    """the eigenvalues a family claims (before the rounding; `graded`: of its unscaled core)"""
    kappa = kappa_of(name, t)
    if name in ("geo", "graded"):
        return np.geomspace(1.0, 1.0 / kappa, n)
    lam = np.full(n, 1.0 / kappa if name == "one_large" else 1.0)
    if name == "one_large":
        lam[0] = 1.0
    else:
        lam[-1] = 1.0 / kappa
    return lam


@functools.lru_cache(maxsize=None)
def grading(t, n, seed=5):
    d = np.logspace(0.0, grading_of(t), n)
    np.random.default_rng(seed + n).shuffle(d)
    return frozen(d)


@functools.lru_cache(maxsize=None)
def family(name, t, n, seed=11):
    """the rounded Hermitian positive definite matrix of one family, read-only, column-major"""
    q = unitary(t, n, seed + n)
    a = (q * spectrum_of(name, t, n)[None, :]) @ q.conj().T
    if name == "graded":
        d = grading(t, n)
        a = d[:, None] * a * d[None, :]
    return frozen(hermitian_rounded(a, t))


@functools.lru_cache(maxsize=None)
def rhs(t, n, nrhs, seed=3):
    rng = np.random.default_rng(seed + n + nrhs)
    b = rng.uniform(-1, 1, (n, nrhs))
    if t in "cz":
        b = b + 1j * rng.uniform(-1, 1, (n, nrhs))
    return frozen(np.asfortranarray(b.astype(DT[t])))


# ------------------------------------------------------------------------------------------------ buffers and bits
def padded(a):
    """(buf, view): `a` in a buffer with a padded leading dimension (n + PAD rows), sentinels in the padding"""
    n = a.shape[0]
    buf = np.full((n + PAD, a.shape[1]), SENTINEL, dtype=a.dtype, order="F")
    buf[:n, :] = a
    return buf, buf[:n, :]


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def tri_mask(n, uplo, strict=False):
    m = np.tril(np.ones((n, n), bool), -1 if strict else 0)
    return m if uplo == "L" else m.T


def untouched(buf, buf0, uplo):
    """everything outside the uplo triangle of the leading n x n part (n = columns), the padding included, bit-identical"""
    n = buf.shape[1]
    outside = np.ones(buf.shape, bool)
    outside[:n, :][tri_mask(n, uplo)] = False
    return same_bits(buf[outside], buf0[outside])


def tri_same_bits(x, y, uplo):
    m = tri_mask(x.shape[0], uplo)
    return same_bits(x[m], y[m])


def lower_of(got, uplo):
    """the lower factor the uplo triangle of `got` holds (upper: its adjoint)"""
    return np.tril(got) if uplo == "L" else np.triu(got).conj().T


def diagonal_ok(got):
    d = np.diagonal(got)
    return bool((d.real > 0).all() and (d.imag == 0).all())


# ----------------------------------------------------------------------------------------------------- the measures
def wide_llh_lower(low, hp):
    """the lower triangle of L L^H in the wide type, by block columns of the triangular factor (a third of the full
    product: numpy has no BLAS for longdouble)"""
    n = low.shape[0]
    lw = low.astype(hp)
    out = np.zeros((n, n), hp)
    step = 128
    for j0 in range(0, n, step):
        j1 = min(j0 + step, n)
        out[j0:, j0:j1] = lw[j0:, :j1] @ lw[j0:j1, :j1].conj().T
    return out


def factor_ratios(t, a, low):
    """(normwise, componentwise) of the lower factor `low` of the rounded matrix `a`, formed in the wide type:
    max|A - L L^H| / (n eps max|A|) and max(|A - L L^H| / (|L||L|^H)) / (n eps), over the lower triangle (the residual
    is Hermitian)"""
    n = a.shape[0]
    hp = WIDE[t]
    low = np.tril(low)
    mask = tri_mask(n, "L")
    res = np.abs(a.astype(hp) - wide_llh_lower(low, hp)).astype(np.float64)
    al = np.abs(low).astype(np.float64)
    bound = al @ al.T  # (a sum of non-negative terms: float64 carries it to 1e-13 of itself)
    ne = n * eps_of(t)
    with np.errstate(invalid="ignore", divide="ignore"):
        comp = np.where(bound[mask] > 0, res[mask] / bound[mask], np.where(res[mask] > 0, np.inf, 0.0))
    return float(res[mask].max() / (ne * np.abs(a).max())), float(comp.max() / ne)


def solve_ratio(t, a, b, x):
    """max_j ||b_j - A x_j||_inf / ((||A||_inf ||x_j||_inf + ||b_j||_inf) n eps), in the wide type"""
    n = a.shape[0]
    hp = WIDE[t]
    r = np.abs(b.astype(hp) - a.astype(hp) @ x.astype(hp)).astype(np.float64).max(axis=0)
    na = float(np.abs(a).astype(np.float64).sum(axis=1).max())
    nx = np.abs(x).astype(np.float64).max(axis=0)
    nb_ = np.abs(b).astype(np.float64).max(axis=0)
    return float((r / ((na * nx + nb_) * n * eps_of(t))).max())


# ------------------------------------------------------------------------------------------- the LAPACK reference
@functools.lru_cache(maxsize=None)
def lapack_factor(name, t, n, uplo):
    """(info, lower factor) of ?potrf in the working precision on the rounded input"""
    c, info = sl.lapack.get_lapack_funcs("potrf", (family(name, t, n),))(family(name, t, n), lower=(uplo == "L"), clean=True)
    return int(info), frozen(lower_of(c, uplo))


@functools.lru_cache(maxsize=None)
def lapack_factor_ratios(name, t, n, uplo):
    info, low = lapack_factor(name, t, n, uplo)
    assert info == 0, (name, t, n, uplo, info)
    return factor_ratios(t, family(name, t, n), low)


@functools.lru_cache(maxsize=None)
def lapack_solve_ratio(name, t, n, nrhs, uplo):
    a, b = family(name, t, n), rhs(t, n, nrhs)
    info, low = lapack_factor(name, t, n, uplo)
    assert info == 0
    c = low if uplo == "L" else low.conj().T
    x = sl.cho_solve((np.asfortranarray(c), uplo == "L"), b)
    assert x.dtype == DT[t]
    return solve_ratio(t, a, b, x)


def calibrate(verbose=True):
    """the worst ratios of the working-precision LAPACK route over the whole input set: what REF_FACTOR and REF_SOLVE
    record"""
    fac = {t: [0.0, 0.0] for t in "scdz"}
    sol = {t: 0.0 for t in "dz"}
    for t in "scdz":
        for n, _ in sizes_of(t):
            for name in FAMILIES:
                for uplo in "LU":
                    r = lapack_factor_ratios(name, t, n, uplo)
                    fac[t] = [max(x, y) for x, y in zip(fac[t], r)]
            if verbose:
                print("factor", t, n, fac[t], flush=True)
    for t in "dz":
        for n, _ in SOLVE_SIZES:
            for name in SOLVE_FAMILIES:
                for nrhs in NRHS:
                    for uplo in "LU":
                        sol[t] = max(sol[t], lapack_solve_ratio(name, t, n, nrhs, uplo))
        if verbose:
            print("solve", t, sol[t], flush=True)
    return fac, sol


# ------------------------------------------------------- the blocked algorithm with inverted diagonal blocks (numpy)
def block_starts(n, nb):
    """the starts of the JB-column blocks: they restart at every tile (nb = 100 gives 64 + 36 per tile)"""
    return [k for t0 in range(0, n, nb) for k in range(t0, min(t0 + nb, n), JB)]


def inverted_block(l11):
    """inv(l11) of a lower triangular block, by substitution in its own precision"""
    return sl.solve_triangular(l11, np.eye(l11.shape[0], dtype=l11.dtype), lower=True).astype(l11.dtype)


def emulate_factor(a, nb, fault=None):
    """The right-looking algorithm in the working precision of `a`: every JB-column diagonal block is factored and
    INVERTED (W = inv(L11)), the panel below it is the product with W^H, and the trailing matrix is updated tile by tile.
    Returns (lower factor, list of W, info); info = 0, or the first column of the diagonal block that was not positive
    definite, plus one.  fault = ("slab", tile_i, tile_j, block): that block's slab is left out of the
    update of tile (tile_i, tile_j); ("w", tile_i, block): the rows of tile_i of that block's panel are formed with W
    where W^H is meant."""
    n = a.shape[0]
    w_ = np.tril(np.array(a, order="F"))
    ws = []
    for b, k0 in enumerate(block_starts(n, nb)):
        k1 = min(k0 + JB, (k0 // nb + 1) * nb, n)
        blk = np.tril(w_[k0:k1, k0:k1])
        try:
            l11 = np.linalg.cholesky(blk + np.tril(blk, -1).conj().T)
        except np.linalg.LinAlgError:
            return np.tril(w_), ws, k0 + 1
        w_[k0:k1, k0:k1] = l11
        w = inverted_block(l11)
        ws.append(w)
        if k1 == n:
            break
        for r0 in range((k1 // nb) * nb, n, nb):
            lo, hi = max(r0, k1), min(r0 + nb, n)
            wrong = fault is not None and fault[0] == "w" and fault[1] == r0 // nb and fault[2] == b
            w_[lo:hi, k0:k1] = w_[lo:hi, k0:k1] @ (w if wrong else w.conj().T)
        p = w_[k1:, k0:k1]
        for ti in range(k1 // nb, -(-n // nb)):
            for tj in range(k1 // nb, ti + 1):
                if fault is not None and fault[0] == "slab" and fault[1:] == (ti, tj, b):
                    continue
                r0, r1 = max(ti * nb, k1), min((ti + 1) * nb, n)
                c0, c1 = max(tj * nb, k1), min((tj + 1) * nb, n)
                w_[r0:r1, c0:c1] -= p[r0 - k1:r1 - k1] @ p[c0 - k1:c1 - k1].conj().T
    return np.tril(w_), ws, 0


def emulate_solve(low, ws, nb, b):
    """A X = B from that factor, both substitutions by JB-row blocks with the inverted diagonal blocks, in the working
    precision"""
    n = low.shape[0]
    x = np.array(b, order="F")
    starts = block_starts(n, nb)
    ends = [min(k0 + JB, (k0 // nb + 1) * nb, n) for k0 in starts]
    for w, k0, k1 in zip(ws, starts, ends):
        x[k0:k1] = w @ x[k0:k1]
        x[k1:] -= low[k1:, k0:k1] @ x[k0:k1]
    for w, k0, k1 in reversed(list(zip(ws, starts, ends))):
        x[k0:k1] = w.conj().T @ (x[k0:k1] - low[k1:, k0:k1].conj().T @ x[k1:])
    return x


# --------------------------------------------------------------------------------------------- scale equivariance
def scale_exponent(t):
    """k of s = 4^k"""
    return 200 if t in "dz" else 20


def in_normal_range(x, t, k):
    """no non-zero real or imaginary part of 2^k x is subnormal or overflows in the working type"""
    f = np.finfo(DT[t])
    parts = np.abs(np.concatenate([np.real(x).ravel(), np.imag(x).ravel()]).astype(np.float64))
    parts = parts[parts > 0]
    if parts.size == 0:
        return True
    lo, hi = np.log2(parts.min()) + k, np.log2(parts.max()) + k
    return bool(lo >= np.log2(float(f.tiny)) and hi < np.log2(float(f.max)))


def scaled(a, k):
    """4^k a, exactly"""
    return np.asfortranarray(np.ldexp(a.real, 2 * k) + (1j * np.ldexp(a.imag, 2 * k) if np.iscomplexobj(a) else 0)).astype(a.dtype)


def times_pow2(x, k):
    """2^k x, exactly"""
    return (np.ldexp(x.real, k) + (1j * np.ldexp(x.imag, k) if np.iscomplexobj(x) else 0)).astype(x.dtype)


# ------------------------------------------------------------------------------------------ not positive definite
def unblocked_pivots(a):
    """The textbook column Cholesky of the lower triangle of `a` in the wide type of its element type.  Returns
    (info, pivots): info = j + 1 for the first pivot that is <= 0 OR NaN (the contract of the drivers: "a non-positive or
    NaN pivot at column c"), else 0; pivots = the pivots met, the failing one included."""
    t = {v: k for k, v in DT.items()}[a.dtype.type]
    hp = WIDE[t]
    n = a.shape[0]
    aw = np.tril(np.asarray(a)).astype(hp)
    low = np.zeros((n, n), hp)
    piv = []
    with np.errstate(all="ignore"):
        for j in range(n):
            row = low[j, :j]
            d = aw[j, j].real - (row.real @ row.real + row.imag @ row.imag)
            piv.append(float(d))
            if not d > 0:
                return j + 1, np.array(piv)
            low[j, j] = np.sqrt(d)
            if j + 1 < n:
                low[j + 1:, j] = (aw[j + 1:, j] - low[j + 1:, :j] @ row.conj()) / low[j, j]
    return 0, np.array(piv)


def unblocked_info(a):
    return unblocked_pivots(a)[0]


def decisive(a):
    """every pivot before the failing one above +1e3 n eps max|A|, the failing one below -1e3 n eps max|A|: rounding
    cannot move the index"""
    info, piv = unblocked_pivots(a)
    n = a.shape[0]
    margin = 1e3 * n * float(np.finfo(a.dtype).eps) * float(np.abs(a).max())
    return bool(info > 0 and (piv[:-1] > margin).all() and piv[-1] < -margin)


def planted(t, n, where, name="one_small"):
    """a family matrix with a[j, j] replaced by -|a[j, j]| for every j of `where`"""
    a = np.array(family(name, t, n), order="F")
    for j in where:
        a[j, j] = -abs(a[j, j])
    return a


# where the eigenvector of the negative eigenvalue carries its weight: (rows of full weight, weight of the others)
THROUGH_SHAPE = {"tile0": (slice(0, 250), 0.02), "tile1": (slice(0, 600), 1.0), "last": (slice(512, 600), 0.3)}
THROUGH_RANGE = {"tile0": (0, 256), "tile1": (256, 512), "last": (512, 600)}
THROUGH_N = 600
# seeds at which the failing index falls in the wanted tile with the decisive margin, in all four types (searched on the
# CPU; test_hard_spd.py asserts both)
THROUGH_SEED = {"tile0": 0, "tile1": 1, "last": 0}


@functools.lru_cache(maxsize=None)
def through_updates(t, where, seed=None):
    """Q diag(lambda) Q^H of order 600 with one eigenvalue -0.5 among eigenvalues in [1, 2]: every diagonal entry is
    positive and a pivot turns negative only through the trailing updates.  The first column of Q (the eigenvector of
    -0.5) is a Gaussian vector weighted by THROUGH_SHAPE[where], which decides the tile in which the leading minors turn
    indefinite; the other columns complete it to a unitary matrix."""
    n = THROUGH_N
    rng = np.random.default_rng(1000 + (THROUGH_SEED[where] if seed is None else seed))
    g = rng.standard_normal((n, n))
    if t in "cz":
        g = g + 1j * rng.standard_normal((n, n))
    rows, rest = THROUGH_SHAPE[where]
    weight = np.full(n, rest)
    weight[rows] = 1.0
    g[:, 0] *= weight
    q = np.linalg.qr(g)[0]
    lam = np.concatenate([[-0.5], rng.uniform(1.0, 2.0, n - 1)])
    return frozen(hermitian_rounded((q * lam[None, :]) @ q.conj().T, t))


def with_value(a, i, j, value):
    """`a` with `value` at (i, j) and at (j, i): the matrix stays symmetric in its positions"""
    out = np.array(a, order="F")
    out[i, j] = value
    out[j, i] = value
    return out


NONFINITE_DIAG = [77, 256]
NONFINITE_OFF = [(150, 20), (400, 20), (599, 300)]
