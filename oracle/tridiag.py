"""tridiag.py -- TEST INFRASTRUCTURE ONLY.

numpy restatement of the reference's eigensolver stages behind reduction_to_band:
band -> tridiagonal, the tridiagonal eigensolver's checks, and the back-transformation band <- tridiagonal.
May be imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg only; the product never imports it.

What it follows (paths relative to /root/reference):
  * BandToTridiag::call_L, local            include/dlaf/eigensolver/band_to_tridiag/mc.h:681-867
      - HH_reflector (xLARFG)               :55-68
      - apply_HH_left_right_herm            :70-86   (xHEMV, w += -1/2 tau (w^H v) v, xHER2)
      - apply_HH_left / apply_HH_right      :88-118
      - SweepWorker::start_sweep / do_step  :503-531
      - nrSweeps / nrStepsForSweep          include/dlaf/eigensolver/band_to_tridiag/api.h:24-34
      - layout of the compact reflectors    include/dlaf/eigensolver/band_to_tridiag.h:40-72, mc.h:762-768
  * the checker of the reference's own test test/unit/eigensolver/test_band_to_tridiag.cpp:60-118
  * bt_band_to_tridiagonal (definition)     include/dlaf/eigensolver/bt_band_to_tridiag.h:28-61: E <- Q E with
                                            Q = HHT(0,0) HHT(0,1) ... HHT(1,0) ... (band_to_tridiag.h:49-53)
  * the checkers of test_tridiag_solver_local.cpp:62-129 (1D Laplacian, closed form) and
    test/include/dlaf_test/eigensolver/test_eigensolver_correctness.h:37-101 (orthogonality, A E = E Lambda)

The arithmetic of HH_reflector is LAPACK's xLARFG (a third-party dependency of the reference, lapackpp >= 2022.05
-> the system LAPACK), restated from its published algorithm without the rescaling loop for subnormal norms.

Pinned by: the reference test's reconstruction property (applying the stored reflectors to the tridiagonal matrix
gives back the band matrix, tolerance of test_band_to_tridiag.cpp:117), LAPACK ?sbtrd-independent spectrum
preservation (eigvalsh(tridiagonal) == eigvalsh(band)), scipy's eigh_tridiagonal and the closed-form 1D Laplacian.
"""
from __future__ import annotations

import numpy as np

from .red2band import error_of


def is_complex(dtype) -> bool:
    return np.dtype(dtype).kind == "c"


def nr_sweeps(n: int, dtype) -> int:
    """api.h:24-28."""
    return n - 1 if is_complex(dtype) else n - 2


def nr_steps_for_sweep(sweep: int, n: int, band: int) -> int:
    """api.h:30-34."""
    return 1 if sweep == n - 2 else -((n - sweep - 2) // -band)


def larfg(x: np.ndarray):
    """xLARFG on x (in place): x[0] <- beta, x[1:] <- v[1:]; returns tau."""
    n = x.shape[0]
    cx = is_complex(x.dtype)
    if n <= 0:
        return x.dtype.type(0)
    alpha = x[0]
    xnorm = np.linalg.norm(x[1:]) if n > 1 else 0.0
    if xnorm == 0 and (not cx or alpha.imag == 0):
        return x.dtype.type(0)
    if cx:
        beta = -np.copysign(np.sqrt(alpha.real ** 2 + alpha.imag ** 2 + xnorm ** 2), alpha.real)
        tau = complex((beta - alpha.real) / beta, -alpha.imag / beta)
    else:
        beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
        tau = (beta - alpha) / beta
    x[1:] *= 1 / (alpha - beta)
    x[0] = beta
    return x.dtype.type(tau)


def band_to_tridiag(a: np.ndarray, band: int):
    """BandToTridiag::call_L on the dense Hermitian band matrix a (lower triangle referenced, bandwidth `band`).
    Returns (d, e, v): diagonal, off-diagonal (length n - 1, real) and the n x n matrix of compact reflectors
    (tau in the place of the leading 1), laid out as band_to_tridiag.h:56-63 says."""
    n = a.shape[0]
    dt = a.dtype
    b = band
    # full Hermitian working copy (the reference works on the lower band only; same arithmetic per element)
    w = np.tril(a).astype(dt)
    w = w + np.tril(w, -1).conj().T
    v_out = np.zeros((n, n), dtype=dt)
    if n == 0:
        return np.zeros(0, dtype=w.real.dtype), np.zeros(0, dtype=w.real.dtype), v_out
    for sweep in range(max(0, nr_sweeps(n, dt))):
        # start_sweep (mc.h:503-508): reflector of column `sweep`, rows sweep+1 ...
        nn = min(n - sweep - 1, b)
        x = w[sweep + 1:sweep + 1 + nn, sweep].copy()
        tau = larfg(x)
        v = x.copy()
        v[0] = 1
        w[sweep + 1, sweep] = x[0]
        w[sweep + 2:sweep + 1 + nn, sweep] = 0
        w[sweep, sweep + 1:sweep + 1 + nn] = w[sweep + 1:sweep + 1 + nn, sweep].conj()
        for step in range(nr_steps_for_sweep(sweep, n, b)):
            j = 1 + sweep + step * b
            nh = min(b, n - j)
            # compact_copy_to_tile (mc.h:492-497, :766-768)
            pos = (sweep // b + step) * b
            v_out[pos, sweep] = tau
            v_out[pos + 1:pos + nh, sweep] = v[1:nh]
            m = min(b, n - b - j)
            # apply_HH_left_right_herm on the nh x nh diagonal block
            d = w[j:j + nh, j:j + nh]
            ww = tau * (d @ v[:nh])
            ww = ww + (-np.vdot(ww, v[:nh]) * tau / 2) * v[:nh]
            d -= np.outer(ww, v[:nh].conj()) + np.outer(v[:nh], ww.conj())
            if m > 0:
                # apply_HH_right on the m x nh block below
                blk = w[j + nh:j + nh + m, j:j + nh]
                wr = blk @ v[:nh]
                blk -= tau * np.outer(wr, v[:nh].conj())
                w[j:j + nh, j + nh:j + nh + m] = blk.conj().T
            if m > 1:
                x = w[j + nh:j + nh + m, j].copy()
                tau = larfg(x)
                v = x.copy()
                v[0] = 1
                w[j + nh, j] = x[0]
                w[j + nh + 1:j + nh + m, j] = 0
                blk = w[j + nh:j + nh + m, j + 1:j + nh]
                wl = blk.conj().T @ v[:m]
                blk -= np.conj(tau) * np.outer(v[:m], wl.conj())
                w[j:j + nh, j + nh:j + nh + m] = w[j + nh:j + nh + m, j:j + nh].conj().T
    d = np.real(np.diag(w)).copy()
    e = np.real(np.diag(w, -1)).copy()
    return d, e, v_out


def reflector_list(n: int, band: int, dtype):
    """(sweep, step, first_row, size, pos) of every reflector in the order of Q = HHT(0,0) HHT(0,1) ...
    (band_to_tridiag.h:49-63)."""
    out = []
    for sweep in range(max(0, nr_sweeps(n, dtype))):
        for step in range(nr_steps_for_sweep(sweep, n, band)):
            first = 1 + sweep + step * band
            size = min(band, n - first)
            out.append((sweep, step, first, size, (sweep // band + step) * band))
    return out


def apply_q(v: np.ndarray, band: int, e: np.ndarray, adjoint: bool = False) -> np.ndarray:
    """E <- Q E (bt_band_to_tridiagonal) or Q^H E, one reflector at a time -- the definition."""
    n = v.shape[0]
    e = e.copy()
    refl = reflector_list(n, band, v.dtype)
    order = refl if adjoint else reversed(refl)
    for sweep, step, first, size, pos in order:
        vec = v[pos:pos + size, sweep].copy()
        tau = vec[0]
        vec[0] = 1
        if adjoint:
            tau = np.conj(tau)
        rows = e[first:first + size]
        rows -= tau * np.outer(vec, vec.conj() @ rows)
    return e


def check_band_to_tridiag(a: np.ndarray, band: int, d: np.ndarray, e: np.ndarray, v: np.ndarray):
    """test_band_to_tridiag.cpp:60-118: rebuild the band matrix from the tridiagonal one and the stored reflectors,
    compare the lower band with the input.  Returns (ok, max abs diff, bar)."""
    n = a.shape[0]
    dt = a.dtype
    t = np.zeros((n, n), dtype=dt)
    t[np.arange(n), np.arange(n)] = d
    if n > 1:
        t[np.arange(1, n), np.arange(n - 1)] = e[:n - 1]
        t[np.arange(n - 1), np.arange(1, n)] = e[:n - 1]
    # A = Q T Q^H
    q_t = apply_q(v, band, t)
    full = apply_q(v, band, q_t.conj().T).conj().T
    mask = np.tril(np.ones((n, n), dtype=bool)) & ~np.tril(np.ones((n, n), dtype=bool), -(band + 1))
    want = np.where(mask, a, 0)
    got = np.where(mask, full, 0)
    nb_like = max(band, 1)
    err = error_of(dt)
    diff = np.abs(got - want)
    # CHECK_MATRIX_NEAR(res, mat_a_h, mb * m * error, m * error): relative or absolute
    rel_ok = diff <= nb_like * n * err * np.maximum(np.abs(want), np.finfo(want.real.dtype).tiny)
    abs_ok = diff <= max(n, 1) * err * max(1.0, float(np.abs(want).max(initial=0)))
    return bool(np.all(rel_ok | abs_ok)), float(diff.max(initial=0)), float(n * err)


def laplace_1d(n: int, dtype=np.float64):
    """test_tridiag_solver_local.cpp:62-129: (d, e, eigenvalues, eigenvectors) of the 1D Laplacian."""
    d = np.full(n, 2, dtype=dtype)
    e = np.full(max(n - 1, 0), -1, dtype=dtype)
    i = np.arange(1, n + 1)
    evals = 2 * (1 - np.cos(np.pi * i / (n + 1)))
    evecs = np.sqrt(2.0 / (n + 1)) * np.sin(np.outer(i, i) * np.pi / (n + 1))
    return d, e, evals.astype(dtype), evecs.astype(dtype)


def check_eigensolver(a_full: np.ndarray, evals: np.ndarray, evecs: np.ndarray):
    """test_eigensolver_correctness.h:37-101 on the full Hermitian matrix a_full: eigenvalues sorted, E^H E == I
    (m * error relative / 10 m error absolute), A E == E Lambda (2 m error).  Returns a dict of the three findings."""
    m = a_full.shape[0]
    err = error_of(evecs.dtype)
    srt = bool(np.all(np.diff(evals) >= 0))
    g = evecs.conj().T @ evecs
    orth = float(np.abs(g - np.eye(m)).max(initial=0))
    ae = a_full @ evecs
    el = evecs * evals[None, :]
    diff = np.abs(ae - el)
    tol = 2 * m * err
    res_ok = bool(np.all((diff <= tol) | (diff <= tol * np.abs(el))))
    return {"sorted": srt, "orth": orth, "orth_bar": 10 * m * err, "residual": float(diff.max(initial=0)),
            "residual_bar": tol, "residual_ok": res_ok}


# ------------------------------------------------------------------ extended-precision reference of the tridiagonal solver
def sturm_eigvals(d: np.ndarray, e: np.ndarray, iters: int = 80) -> np.ndarray:
    """All eigenvalues (ascending, np.longdouble) of the symmetric tridiagonal matrix with diagonal d and off-diagonal
    e[:n - 1], by Sturm-count bisection in 80-bit long double from the Gershgorin bounds: `iters` halvings of every
    bracket at once (one numpy operation per row on all n brackets), a bracket of width (hi - lo) 2^-iters at the end.
    A zero pivot of the LDL^T recurrence is replaced by `tiny`."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18, "sturm_eigvals needs an 80-bit long double (x87): this platform has none"
    d = np.asarray(d).astype(ld)
    n = d.shape[0]
    if n == 0:
        return np.zeros(0, dtype=ld)
    e = np.asarray(e).astype(ld)[:n - 1]
    ae = np.abs(e)
    r = np.zeros(n, dtype=ld)
    r[:-1] += ae
    r[1:] += ae
    lo0, hi0 = np.min(d - r), np.max(d + r)
    pad = (hi0 - lo0 + max(abs(lo0), abs(hi0))) * np.finfo(ld).eps * 4 * n
    lo = np.full(n, lo0 - pad, dtype=ld)
    hi = np.full(n, hi0 + pad, dtype=ld)
    if hi0 == lo0 == 0:
        return np.zeros(n, dtype=ld)
    k = np.arange(n)
    e2 = e * e
    tiny = np.finfo(ld).tiny
    q, t = np.empty(n, dtype=ld), np.empty(n, dtype=ld)
    neg = np.empty(n, dtype=bool)
    cnt = np.empty(n, dtype=np.int64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for _ in range(iters):
            x = lo + (hi - lo) / 2
            np.subtract(d[0], x, out=q)
            if not q.all():
                q[q == 0] = tiny
            np.less(q, 0, out=neg)
            cnt[:] = neg
            for i in range(1, n):
                np.divide(e2[i - 1], q, out=t)
                np.subtract(d[i], x, out=q)
                q -= t
                if not q.all():
                    q[q == 0] = tiny
                np.less(q, 0, out=neg)
                cnt += neg
            # cnt = number of eigenvalues below x
            above = cnt > k
            hi = np.where(above, x, hi)
            lo = np.where(above, lo, x)
    return lo + (hi - lo) / 2


def check_tridiag_solution(d, e, w, z, dtype, w_ref=None) -> dict:
    """Findings of a tridiagonal eigensolver's (w, z) for the tridiagonal matrix T = (d, e), all relative to
    |T|_2 = max |w_ref| (w_ref: sturm_eigvals(d, e) unless given) and in units of eps of `dtype`: sorted,
    eig = max |w - w_ref| / (eps |T|), residual = max_j |T z_j - w_j z_j|_inf / (eps |T|) (long double), orth =
    max |Z^T Z - I| / eps (float64 products)."""
    ld = np.longdouble
    eps = float(np.finfo(dtype).eps)
    n = len(d)
    if w_ref is None:
        w_ref = sturm_eigvals(d, e)
    tn = float(np.abs(w_ref).max(initial=0))
    unit = eps * tn if tn > 0 else np.finfo(np.float64).tiny
    wl = np.asarray(w).astype(ld)
    out = {"n": n, "norm": tn, "sorted": bool(np.all(np.diff(wl) >= 0)),
           "eig": float(np.abs(wl - np.asarray(w_ref, dtype=ld)).max(initial=0)) / unit}
    dl = np.asarray(d).astype(ld)
    el = np.asarray(e).astype(ld)[:max(n - 1, 0)]
    res = []  # per chunk of columns; np.max of them lets a NaN through (the built-in max would drop it)
    for c0 in range(0, n, 256):
        zl = np.asarray(z[:, c0:c0 + 256]).astype(ld)
        tz = dl[:, None] * zl
        tz[:-1] += el[:, None] * zl[1:]
        tz[1:] += el[:, None] * zl[:-1]
        tz -= zl * wl[None, c0:c0 + 256]
        res.append(np.abs(tz).max(initial=0))
    out["residual"] = float(np.max(res, initial=0)) / unit
    z64 = np.asarray(z, dtype=np.float64)
    out["orth"] = float(np.abs(z64.T @ z64 - np.eye(n)).max(initial=0)) / eps
    return out


LEAF = 64  # the solver's default leaf size: its merge boundaries are at rows 64 j - 1 / 64 j

FAMILIES = ["zero", "const", "diag", "rand_neg", "rand_alt", "rand_mixed", "clement", "wilkinson", "glued_wilk_1e-14",
            "glued_wilk_sqrteps", "graded", "dlatms_a", "dlatms_b", "dlatms_c", "dlatms_d", "dlatms_e", "rho0",
            "zero_e_inside", "repeated"]


def _wilkinson(m: int):
    """W+ of order m: d_i = |(m - 1)/2 - i|, e = 1 (W+_{2k+1} for odd m)."""
    return np.abs((m - 1) / 2 - np.arange(m)), np.ones(max(m - 1, 0))


def _glued(block: int, n: int, glue_rel: float):
    bd, be = _wilkinson(block)
    bn = float(np.abs(np.linalg.eigvalsh(np.diag(bd) + np.diag(be, 1) + np.diag(be, -1))).max())
    reps = -(-n // block)
    d = np.tile(bd, reps)[:n]
    e = np.tile(np.append(be, bn * glue_rel), reps)[:max(n - 1, 0)]
    return d, e


def _dlatms(mode: str, n: int, dtype, rng):
    """Q Lambda Q^T (Q Haar-distributed) reduced to tridiagonal form in float64 (LAPACK dsytrd), Lambda of the
    xLATMS modes with kappa = 1/eps of `dtype` and random signs."""
    import scipy.linalg as sl
    kappa = 1 / float(np.finfo(dtype).eps)
    i = np.arange(n)
    if mode == "a":
        lam = np.full(n, 1 / kappa)
        lam[0] = 1
    elif mode == "b":
        lam = np.ones(n)
        lam[-1] = 1 / kappa
    elif mode == "c":
        lam = kappa ** (-i / max(n - 1, 1))
    elif mode == "d":
        lam = 1 - i / max(n - 1, 1) * (1 - 1 / kappa)
    else:
        lam = np.exp(-rng.uniform(0, np.log(kappa), n))
    lam = lam * rng.choice([-1.0, 1.0], n)
    if n == 1:
        return lam.copy(), np.zeros(0)
    q, rr = np.linalg.qr(rng.standard_normal((n, n)))
    q *= np.sign(np.diag(rr))[None, :]
    a = (q * lam[None, :]) @ q.T
    a = (a + a.T) / 2
    _, dd, ee, _, info = sl.lapack.dsytrd(a, lower=1)
    assert info == 0
    return dd, ee


def tridiag_family(name: str, n: int, dtype, seed: int = 0):
    """(d, e) of the named test-matrix family (FAMILIES), in `dtype`, e of length max(n - 1, 0).  Deterministic in
    (name, n, dtype, seed).  The classes of the LAPACK xSTEDC tester (xCHKST: zero, constant / random diagonal,
    Clement, Wilkinson, glued Wilkinson, xLATMS spectra) and of the tridiagonal test-set literature (graded), plus
    the structures of this solver's divide & conquer tree (leaves of LEAF rows): rho = 0 at merge boundaries, zero
    couplings inside leaves, repeated blocks whose merges tie."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, n, sum(map(ord, name)), dtype.itemsize])
    m = max(n - 1, 0)
    eps = float(np.finfo(dtype).eps)
    if name == "zero":
        d, e = np.zeros(n), np.zeros(m)
    elif name == "const":
        d, e = np.full(n, -0.3), np.zeros(m)
    elif name == "diag":
        d, e = rng.permutation(np.linspace(-1, 1, n) + rng.uniform(0, 0.5 / max(n, 1), n)), np.zeros(m)
    elif name.startswith("rand_"):
        d = rng.uniform(-1, 1, n)
        e = rng.uniform(0.05, 1, m)
        if name == "rand_neg":
            e = -e
        elif name == "rand_alt":
            e = e * (-1.0) ** np.arange(m)
        else:
            e = e * rng.choice([-1.0, 1.0], m)
    elif name == "clement":
        i = np.arange(1, n)
        d, e = np.zeros(n), np.sqrt(i * (n - i))
    elif name == "wilkinson":
        d, e = _wilkinson(n)
    elif name == "glued_wilk_1e-14":
        d, e = _glued(21, n, 1e-14)
    elif name == "glued_wilk_sqrteps":
        d, e = _glued(21, n, np.sqrt(eps))
    elif name == "graded":
        # d_i = 2^(-i s), e_i = 2^(-(i + 1/2) s): the smallest entry stays two binades above the smallest normal number
        span = -np.log2(float(np.finfo(dtype).tiny)) - 2
        s = span / max(n - 1, 1)
        i = np.arange(n, dtype=np.float64)
        d, e = 2.0 ** (-i * s), 2.0 ** (-(i[:m] + 0.5) * s)
    elif name.startswith("dlatms_"):
        d, e = _dlatms(name[-1], n, dtype, rng)
    elif name == "rho0":
        d, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
        e[LEAF - 1::LEAF] = 0
    elif name == "zero_e_inside":
        d, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
        for r in (10, 31, 32, 62):
            e[r::LEAF] = 0
    elif name == "repeated":
        bd, be = rng.uniform(-1, 1, LEAF), rng.uniform(-1, 1, LEAF - 1)
        bn = float(np.abs(np.linalg.eigvalsh(np.diag(bd) + np.diag(be, 1) + np.diag(be, -1))).max())
        glue = eps * 2.0 ** np.ceil(np.log2(bn))
        reps = -(-n // LEAF)
        d = np.tile(bd, reps)[:n]
        e = np.tile(np.append(be, glue), reps)[:m]
    else:
        raise ValueError(f"unknown family {name}")
    return np.asarray(d, dtype=dtype), np.asarray(e, dtype=dtype)


# ------------------------------------------------------------------ long-double checkers of band -> tridiagonal
# Each returns (ratio to its bar, where): a stage passes when ratio <= 1.  A NaN anywhere makes the ratio NaN (which
# fails `ratio <= 1`); there is no absolute floor, so a matrix of any scale is held to its own norm.
def _ld_type(dtype):
    return np.clongdouble if is_complex(dtype) else np.longdouble


def _eps(dtype) -> float:
    return float(np.finfo(np.zeros(0, dtype=dtype).real.dtype).eps)


def _ratio(err, bar) -> float:
    err = float(err)
    if err != err:
        return float("nan")
    if bar > 0:
        return err / bar
    return 0.0 if err == 0 else float("inf")


def hermitian_band_matmul(a: np.ndarray, band: int, x: np.ndarray):
    """(A x, |A|_F) in long double, A the Hermitian band matrix of the lower band of `a` (the diagonal's imaginary part
    dropped), one diagonal at a time."""
    n = a.shape[0]
    ldt = _ld_type(a.dtype)
    diag = np.diagonal(a).real.astype(np.longdouble)
    y = diag[:, None] * x
    fro = np.sum(diag ** 2)
    for o in range(1, min(band, n - 1) + 1):
        sub = np.diagonal(a, -o).astype(ldt)  # A(i + o, i)
        y[o:] += sub[:, None] * x[:n - o]
        y[:n - o] += sub.conj()[:, None] * x[o:]
        fro += 2 * np.sum(np.abs(sub) ** 2)
    return y, np.sqrt(fro)


def b2t_backward_error(a: np.ndarray, band: int, d, e, v, nprobe: int = 8, seed: int = 0):
    """|A X - Q T Q^H X|_F / (n eps |A|_F |X|_F) on `nprobe` random probe columns X, in long double (A: the Hermitian
    band matrix of the lower band of `a`, Q from v by apply_q)."""
    n = a.shape[0]
    if n == 0:
        return 0.0, "n = 0"
    ldt = _ld_type(a.dtype)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, nprobe))
    if is_complex(a.dtype):
        x = x + 1j * rng.standard_normal((n, nprobe))
    x = x.astype(ldt)
    vl = np.asarray(v).astype(ldt)
    dl = np.asarray(d).astype(np.longdouble)
    el = np.asarray(e).astype(np.longdouble)[:n - 1]
    y = apply_q(vl, band, x, adjoint=True)
    ty = dl[:, None] * y
    ty[:-1] += el[:, None] * y[1:]
    ty[1:] += el[:, None] * y[:-1]
    ax, an = hermitian_band_matmul(a, band, x)
    r = ax - apply_q(vl, band, ty)
    xn = np.sqrt(np.sum(np.abs(x) ** 2))
    err = np.sqrt(np.sum(np.abs(r) ** 2))
    if not (np.all(np.isfinite(dl)) and np.all(np.isfinite(el)) and np.all(np.isfinite(vl))):
        err = float("nan")
    return _ratio(err, n * _eps(a.dtype) * float(an) * float(xn)), f"|A X - Q T Q^H X| = {float(err):.3e}"


def b2t_reflector_unitarity(v, band: int, c: float = 2.0):
    """max over the reflector slots of |2 Re tau - |tau|^2 v^H v| / (c (b + 8) eps): H = I - tau v v^H is unitary exactly
    when that is zero (b eps for the sum v^H v, 8 eps for rounding the stored tau, |tau| <= 2, itself).  `where` names the
    worst (sweep, step)."""
    v = np.asarray(v)
    n = v.shape[0]
    bar = c * (band + 8) * _eps(v.dtype)
    worst, where = 0.0, "no reflector"
    for sweep, step, first, size, pos in reflector_list(n, band, v.dtype):
        col = v[pos:pos + size, sweep].astype(_ld_type(v.dtype))
        tau = col[0]
        vhv = 1 + np.sum(np.abs(col[1:]) ** 2)
        dev = float(abs(2 * tau.real - abs(tau) ** 2 * vhv))
        if dev != dev:
            return float("nan"), f"NaN in the reflector of (sweep {sweep}, step {step})"
        if dev > worst or where == "no reflector":
            worst, where = dev, f"(sweep {sweep}, step {step})"
    return _ratio(worst, bar), where


def b2t_layout(v, band: int, d, e):
    """v is exactly zero outside the reflector slots of reflector_list, and d, e are finite: ratio 0 when so, inf (or NaN)
    when not."""
    v = np.asarray(v)
    n = v.shape[0]
    slot = np.zeros((n, n), dtype=bool)
    for sweep, step, first, size, pos in reflector_list(n, band, v.dtype):
        slot[pos:pos + size, sweep] = True
    stray = np.argwhere(~slot & (v != 0))
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(e))):
        return float("nan"), "d or e not finite"
    if stray.size:
        r, c = stray[0]
        return float("inf"), f"{len(stray)} entries of v outside the slots, first ({r}, {c}) = {v[r, c]}"
    if not np.all(np.isfinite(v)):
        return float("nan"), "v not finite"
    return 0.0, "layout ok"


def b2t_spectrum(a: np.ndarray, band: int, d, e, iters: int = 64, sturm_max: int = 400):
    """max |eig(T) - eig(A)| / (n eps |A|_2): eig(A) by LAPACK in fp64 on A / 2^k (eigvals_banded), so that no scale of A
    over- or underflows it; |A|_2 = max |eig(A)|.  eig(T) by sturm_eigvals (long double) up to n = sturm_max, beyond it
    (where the bisection takes seconds per matrix) by LAPACK in fp64 on T / 2^k."""
    import scipy.linalg as sl
    n = a.shape[0]
    if n == 0:
        return 0.0, "n = 0"
    if not (np.all(np.isfinite(d)) and np.all(np.isfinite(e))):
        return float("nan"), "d or e not finite"
    cx = is_complex(a.dtype)
    wide = np.complex128 if cx else np.float64
    mx = 0.0
    ab = np.zeros((band + 1, n), dtype=wide)
    for o in range(min(band, n - 1) + 1):
        diag = np.diagonal(a, -o).astype(wide)
        ab[o, :n - o] = diag
        mx = max(mx, float(np.abs(diag.real).max(initial=0)), float(np.abs(diag.imag).max(initial=0)) if cx else 0.0)
    ab[0] = ab[0].real
    k = int(np.frexp(mx)[1]) if mx > 0 else 0
    ab = np.ldexp(ab.real, -k) + 1j * np.ldexp(ab.imag, -k) if cx else np.ldexp(ab, -k)
    ref = np.sort(sl.eigvals_banded(ab, lower=True).astype(np.longdouble)) * np.longdouble(2) ** k
    if n <= sturm_max:
        got = sturm_eigvals(d, e, iters=iters)
    else:
        kt = int(np.frexp(max(float(np.abs(d).max(initial=0)), float(np.abs(e).max(initial=0))))[1])
        got = sl.eigvalsh_tridiagonal(np.ldexp(np.asarray(d, dtype=np.float64), -kt),
                                      np.ldexp(np.asarray(e, dtype=np.float64)[:n - 1], -kt),
                                      ).astype(np.longdouble) * np.longdouble(2) ** kt
    anorm = float(np.abs(ref).max(initial=0))
    err = float(np.abs(got - ref).max(initial=0))
    return _ratio(err, n * _eps(a.dtype) * anorm), f"max |eig(T) - eig(A)| = {err:.3e}, |A|_2 = {anorm:.3e}"


def b2t_checks(a: np.ndarray, band: int, d, e, v) -> dict:
    """The four checkers at once: {name: (ratio, where)}."""
    return {"backward": b2t_backward_error(a, band, d, e, v), "unitarity": b2t_reflector_unitarity(v, band),
            "layout": b2t_layout(v, band, d, e), "spectrum": b2t_spectrum(a, band, d, e)}


def b2t_failures(checks: dict) -> dict:
    """The findings of b2t_checks that do not pass (ratio > 1 or NaN)."""
    return {k: r for k, r in checks.items() if not r[0] <= 1}
