"""Operands with real off-diagonal coupling for generalized_to_standard, their wide-precision reference, the one checker
every result goes through, and a numpy emulation of the two phases of csrc/host/gen_to_std.cpp.  A plain module: the GPU
tests (tests/test_gpu_gen_to_std.py), the grid worker (tests/dist_worker.py) and the CPU half (tests/test_hegst_cases.py)
import it.

coupled_case(t, n, seed): A Hermitian with entries uniform(-1, 1) (complex: both parts) and a real diagonal;
B = G G^H / n + 2 I with G of the same kind.  The factor L of B is computed in the wide type (float64 / complex128 for
s / c, np.longdouble / np.clongdouble for d / z; where long double is no wider, float64 -- the rule of
tests/test_gpu_trsm_kernel.py) and rounded ONCE to the working type; for uplo U the stored factor is L^H.  The reference
C = L^-1 A L^-H is computed in the wide type FROM THE ROUNDED FACTOR by row-wise substitution, so the factor's rounding
is no part of the error, and mag = |L^-1| |A| |L^-H| in float64.  The other triangle of A and of the factor holds -9.9.

ratio(got, case, uplo) = max over EVERY element of the uplo triangle of |got - C| / (u mag), u the unit roundoff; no
element is left out and there is no absolute floor beyond a denormal guard.

The bar is anchored to the reference: rho_ref is the ratio of oracle.gen_to_std_local (the restatement of
GenToStd::call_L) run in the working precision on the same operands, and a result passes when
ratio <= 16 max(rho_ref, 4).  The 16 covers what the GPU path does differently from the reference's substitution: 64-wide
products with inverted diagonal blocks, a K = 2 nb two-segment update and other summation orders (the (K + 66) against
(K + 1) constants derived in tests/test_gpu_trsm_kernel.py)."""
import functools
import hashlib

import numpy as np

from test_gpu_trsm_kernel import DT, JUNK, WIDE

JB = 64
MARGIN = 16
RHO_FLOOR = 4


def unit_roundoff(t):
    return float(np.finfo(DT[t]).eps) / 2


def bar(rho_ref):
    return MARGIN * max(rho_ref, RHO_FLOOR)


def draw(rng, shape, cx):
    v = rng.uniform(-1, 1, size=shape)
    return v + 1j * rng.uniform(-1, 1, size=shape) if cx else v


def wide_cholesky(b):
    """The lower Cholesky factor of b, column by column in b's own type."""
    n = b.shape[0]
    l = np.zeros_like(b)
    for j in range(n):
        v = b[j:, j] - l[j:, :j] @ np.conj(l[j, :j])
        d = np.sqrt(v[0].real)
        l[j, j] = d
        l[j + 1:, j] = v[1:] / d
    return l


def wide_forward(l, rhs):
    """inv(l) rhs by row-wise substitution in l's type (l lower triangular)."""
    x = np.zeros(rhs.shape, dtype=l.dtype)
    for i in range(l.shape[0]):
        x[i] = (rhs[i] - l[i, :i] @ x[:i]) / l[i, i]
    return x


_REFERENCES = {}


def reference_from_factor(t, a_full, l_dt):
    """(C, mag) for the Hermitian a_full and the lower factor l_dt, both in the working type: C = L^-1 A L^-H in the wide
    type by row-wise substitution, mag = |L^-1| |A| |L^-H| in float64.  Cached on the operands' bytes."""
    key = (t, hashlib.sha1(np.ascontiguousarray(a_full).tobytes()).hexdigest(),
           hashlib.sha1(np.ascontiguousarray(l_dt).tobytes()).hexdigest())
    if key not in _REFERENCES:
        hp = WIDE[t]
        lw = np.tril(l_dt).astype(hp)
        x = wide_forward(lw, a_full.astype(hp))            # L^-1 A
        c = np.conj(wide_forward(lw, np.conj(x.T))).T      # (L^-1 (L^-1 A)^H)^H
        li = np.abs(np.linalg.inv(np.tril(l_dt).astype(np.complex128 if t in "cz" else np.float64)))
        mag = li @ np.abs(a_full).astype(np.float64) @ li.T
        _REFERENCES[key] = (c, mag)
    return _REFERENCES[key]


class Case:
    """One coupled case: t, n, a (Hermitian, full), b (= rounded B, full), l (the rounded lower factor); c and mag on
    first use (they take the time)."""

    def __init__(self, t, n, a, b, l):
        self.t, self.n, self.a, self.b, self.l = t, n, a, b, l

    @functools.cached_property
    def _ref(self):
        return reference_from_factor(self.t, self.a, self.l)

    @property
    def c(self):
        return self._ref[0]

    @property
    def mag(self):
        return self._ref[1]

    def with_factor(self, stored, uplo):
        """The same A with the factor a library call returned (in the uplo triangle of `stored`): the reference is built
        from that factor."""
        l = np.tril(stored) if uplo == "L" else np.conj(np.triu(stored)).T
        return Case(self.t, self.n, self.a, self.b, np.ascontiguousarray(l))


def poisoned(full, uplo):
    """A copy with -9.9 in the triangle the call must not read (Fortran order)."""
    out = np.array(full, order="F")
    out[np.triu_indices(full.shape[0], 1) if uplo == "L" else np.tril_indices(full.shape[0], -1)] = JUNK
    return out


def a_operand(case, uplo):
    return poisoned(case.a, uplo)


def b_operand(case, uplo):
    return poisoned(case.b, uplo)


def factor_operand(case, uplo):
    return poisoned(case.l if uplo == "L" else np.conj(case.l).T, uplo)


def seed_of(n):
    return 4000 + n


@functools.lru_cache(maxsize=None)
def coupled_case(t, n, seed):
    cx, dt, hp = t in "cz", DT[t], WIDE[t]
    rng = np.random.default_rng(seed)
    m = draw(rng, (n, n), cx).astype(dt)
    a = np.tril(m) + np.conj(np.tril(m, -1)).T
    a[np.arange(n), np.arange(n)] = a[np.arange(n), np.arange(n)].real
    g = draw(rng, (n, n), cx).astype(dt).astype(np.complex128 if cx else np.float64)
    bw = g @ np.conj(g).T / n + 2 * np.eye(n)
    bw = (np.tril(bw) + np.conj(np.tril(bw, -1)).T).astype(hp)
    l = wide_cholesky(bw).astype(dt)
    b = bw.astype(dt)
    b[np.arange(n), np.arange(n)] = b[np.arange(n), np.arange(n)].real
    for arr in (a, b, l):
        arr.setflags(write=False)
    return Case(t, n, a, b, l)


def in_triangle(n, uplo):
    return np.tril(np.ones((n, n), dtype=bool)) if uplo == "L" else np.triu(np.ones((n, n), dtype=bool))


def ratio(got, case, uplo):
    """max over every element of the uplo triangle of |got - C| / (u mag); inf when an element is not finite."""
    keep = in_triangle(case.n, uplo)
    if not np.all(np.isfinite(got[keep])):
        return float("inf")
    diff = np.abs(got.astype(WIDE[case.t]) - case.c).astype(np.float64)
    den = np.maximum(unit_roundoff(case.t) * case.mag, float(np.finfo(DT[case.t]).tiny))
    return float((diff / den)[keep].max())


_RHO = {}


def rho_ref(oracle, case, uplo, nb):
    """The ratio of the oracle's restatement of GenToStd::call_L in the working precision on the case's operands."""
    key = (id(case), uplo, nb)
    if key not in _RHO:
        ref = a_operand(case, uplo)
        oracle.gen_to_std_local(uplo, ref, factor_operand(case, uplo), nb)
        _RHO[key] = (ratio(ref, case, uplo), case)   # (the case is kept alive: its id is the key)
    return _RHO[key][0]


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


def other_triangle_untouched(got, a_in, uplo):
    n = got.shape[0]
    idx = np.triu_indices(n, 1) if uplo == "L" else np.tril_indices(n, -1)
    return same_bits(got[idx], a_in[idx])


def verdict(got, case, uplo, nb, rho, label):
    """(ok, message): the one check of a result.  Prints ratio and rho_ref of the case."""
    r = ratio(got, case, uplo)
    print(f"{label} {case.t}{uplo} n={case.n} nb={nb}: ratio {r:.2f} rho_ref {rho:.2f} bar {bar(rho):.1f}", flush=True)
    if not other_triangle_untouched(got, a_operand(case, uplo), uplo):
        return False, f"{label} {case.t}{uplo} n={case.n} nb={nb}: the other triangle of A changed"
    if not r <= bar(rho):
        return False, (f"{label} {case.t}{uplo} n={case.n} nb={nb}: max |got - C| / (u mag) = {r:.3g} exceeds "
                       f"16 max(rho_ref = {rho:.3g}, 4) = {bar(rho):.3g}")
    return True, ""


def check(got, case, uplo, nb, rho, label):
    ok, msg = verdict(got, case, uplo, nb, rho, label)
    assert ok, msg


# ---- the two phases of csrc/host/gen_to_std.cpp in the working precision ------------------------------------------------
FAULTS = ("segment2", "step4", "phase2", "full_d", "stale", "noconj")


def fault_applies(fault, t, n, nb):
    nt = -(-n // nb)
    if fault in ("phase2", "stale"):
        return nt >= 3
    if fault == "noconj":
        return t in "cz" and nt >= 2
    return nt >= 2


def solve_rh(b, l):
    """X with X l^H = b the way the panel TRSM does it: 64-column steps, the diagonal blocks through their inverses."""
    n = l.shape[0]
    x = b.copy()
    for j0 in range(0, n, JB):
        c = slice(j0, min(n, j0 + JB))
        y = x[:, c] - x[:, :j0] @ np.conj(l[c, :j0]).T
        w = np.linalg.inv(np.tril(l[c, c]))
        x[:, c] = y @ np.conj(w).T
    assert x.dtype == b.dtype
    return x


def hermitian_image(tile):
    h = np.tril(tile) + np.conj(np.tril(tile, -1)).T
    d = np.arange(h.shape[0])
    h[d, d] = h[d, d].real
    return h


def emulate(a_in, fac, uplo, nb, fault=None):
    """The result buffer generalized_to_standard(uplo, a_in, fac, nb) would leave, computed as the header of
    gen_to_std.cpp states the two phases, in the operands' precision.  fault: None or one of FAULTS."""
    n = a_in.shape[0]
    if uplo == "U":   # the transposed view: B^T = L'^-1 A^T L'^-H with L' = U^T
        low = emulate(np.asfortranarray(a_in.T), np.asfortranarray(fac.T), "L", nb, fault)
        out = a_in.copy(order="F")
        iu = np.triu_indices(n)
        out[iu] = low.T[iu]
        return out
    dt = a_in.dtype.type
    a = a_in.copy(order="F")
    nt = -(-n // nb)

    def tl(m, i, j):
        return m[i * nb:min(n, (i + 1) * nb), j * nb:min(n, (j + 1) * nb)]

    far = 2 if nt >= 3 else 1     # the tile row a fault goes into
    stale = None
    for k in range(nt):
        # (1) the diagonal tile: two TRSM passes on the full Hermitian image
        akk, lkk = tl(a, k, k), np.tril(tl(fac, k, k))
        x = solve_rh(hermitian_image(akk), lkk)                        # D L^-H
        x = solve_rh(np.ascontiguousarray(np.conj(x).T), lkk)           # (L^-1 D L^-H)^H
        il = np.tril_indices(akk.shape[0])
        akk[il] = np.conj(x).T[il]
        hs = (dt(1.0) if (fault == "full_d" and k == 0) else dt(0.5)) * hermitian_image(akk)
        # (2) the panel: solve, then the first half-hemm
        for i in range(k + 1, nt):
            src = stale if (fault == "stale" and k == 1 and i == nt - 1) else tl(a, i, k)
            tl(a, i, k)[...] = solve_rh(src, lkk) - tl(fac, i, k) @ hs
        if fault == "stale" and k == 0 and nt >= 3:
            stale = tl(a, nt - 1, 1).copy()
        # (3) the trailing matrix: one K = 2 nb product per tile, the triangle mask on the diagonal tiles
        for j in range(k + 1, nt):
            for i in range(j, nt):
                left = np.concatenate([tl(a, i, k), tl(fac, i, k)], axis=1)
                right = np.concatenate([tl(fac, j, k), tl(a, j, k)], axis=1)
                if fault == "segment2" and k == 0 and (i, j) == (far, 1):
                    left, right = tl(a, i, k), tl(fac, j, k)
                upd = left @ np.conj(right).T
                if i == j:
                    ilj = np.tril_indices(upd.shape[0])
                    tl(a, j, j)[ilj] -= upd[ilj]
                else:
                    tl(a, i, j)[...] -= upd
        # (4) the second half-hemm
        if not (fault == "step4" and k == 0):
            for i in range(k + 1, nt):
                tl(a, i, k)[...] -= tl(fac, i, k) @ hs
    # Phase II by tile rows through the adjoint tiles
    for j in range(1, nt):
        ljj = np.tril(tl(fac, j, j))
        tw = []
        for c in range(j):
            tc = solve_rh(np.ascontiguousarray(np.conj(tl(a, j, c)).T), ljj)
            tw.append(tc)
            tl(a, j, c)[...] = tc.T if fault == "noconj" else np.conj(tc).T
        for i in range(j + 1, nt):
            for c in range(j):
                if fault == "phase2" and (i, j, c) == (2, 1, 0):
                    continue
                tl(a, i, c)[...] -= tl(fac, i, j) @ np.conj(tw[c]).T
    assert a.dtype == a_in.dtype
    return a
