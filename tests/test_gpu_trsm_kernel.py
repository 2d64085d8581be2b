"""The panel TRSM (launch_trsm, csrc/device/kernels_trsm.hip and trsm_rows_z.hpp) and the diagonal-block inversion that
feeds it (launch_invert_diag_blocks / launch_potrf_diag(factor = false), potrf_diag_core.hpp) called directly, one TRSM
launch per case, through dlaf.trsm_direct, against a plain numpy reference written from the contract in
csrc/device/device_api.hpp and not from the kernels: for each local tile il of [il0, il1) the row extent comes from the
global index il pr + ri (last_rows when it is nt - 1, nb otherwise) and X L^H = B (X U^H = B) is solved column by column
in a wider type (float64 for s / c, np.longdouble / np.clongdouble for d / z; where long double is no wider, float64).
Every case asserts the kernel trsm_path chose, so a shape that stops qualifying for a row-owner kernel fails.

Every B buffer is pre-filled with a sentinel: rows past a tile's extent, the rows between the extent and ldb, the gap
between tiles (b_ts > ldb n), a whole tile behind il1 and everything when *info != 0 must come back bit for bit.  The
other triangle of L holds -9.9, L has ldl > n where alignment allows.

Two kinds of operands, neither with a measured tolerance:

* exact (equality).  Built backwards: X has multiples of 2^-3 in [-1, 1]; the off-diagonal 64 x 64 blocks of L are dense
  with the same kind of entries; each diagonal block is D1 (I + N) D2 with D1, D2 diagonal powers of two (with `unit`:
  D2 = inv(D1)) and N strictly triangular, sparse, with small (Gaussian) integer entries, its seed searched for on the
  CPU so that inv(I + N) -- always an integer matrix -- has entries of magnitude <= 8; B = X L^H in the wide type.  Then
  winv, every Y_j = B_j - sum X_p L_jp^H, every X_j = Y_j W_j^H and every partial sum in any order are exactly
  representable.  reference() asserts it: at each step (B and Y_j, Y_j W_j^H, the products L W and W (L W) inside the
  inversion) the sum of the absolute values of the terms divided by their common power-of-two unit (the product of the
  operands' units, an under-estimate of the true unit) stays below 2^24 (s / c) or 2^53 (d / z), and the solve in the
  wide type must return the X the case was built from.  Every element of X and every winv block the device produced
  (the other triangle and everything past jb exactly zero) must be EQUAL to the reference.

* uniform (component-wise bound).  Diagonal entries of magnitude in [1, 2], everything else of the triangle
  uniform(-1, 1) / 8; winv is supplied by the caller: the wide-precision inverse of each diagonal block rounded once.
  With R_j = B_j - Xh L_{j,.}^H the residual of block column j formed in the wide type from the kernel's Xh, K_j the
  number of columns solved before it, G_j = |B_j| + |Xh_solved| |L_{j,solved}|^H, u the unit roundoff and c = 1 (real)
  or 4 (complex, the constant of a complex multiply-add written as real ones, as in test_gpu_update_kernel.py):

      |R_j| <= c (K_j + 66) u  G_j (|W_j|^H |L_jj|^H).

  Derivation.  The kernel forms Yh_j = fl(B_j - sum_{k solved} Xh_k conj(L_jk)): inner products of length K_j and one
  subtraction, in any order: Yh_j = B_j - Xh_s L_js^H + E1, |E1| <= gamma_{K_j+1} G_j, hence |Yh_j| <= (1 + gamma) G_j.
  Then Xh_j = fl(Yh_j Wh_j^H), inner products of length <= 64: Xh_j = Yh_j Wh_j^H + E2, |E2| <= gamma_64 |Yh_j| |W_j|^H.
  Wh_j = W_j + dW, |dW| <= u |W_j|, W_j L_jj = I up to the wide precision.  So
  R_j = B_j - Xh_s L_js^H - Xh_j L_jj^H = (Yh_j - E1) - (Yh_j W_j^H + Yh_j dW^H + E2) L_jj^H
      = -E1 - (Yh_j dW^H + E2) L_jj^H,
  |R_j| <= gamma_{K_j+1} G_j + (u + gamma_64) (1 + gamma) G_j |W_j|^H |L_jj|^H, and because |W|^H |L|^H >= |W^H L^H| = I
  component-wise the first term is below gamma_{K_j+1} G_j |W_j|^H |L_jj|^H: altogether (K_j + 1 + 64 + 1) u = (K_j + 66) u
  up to second order, times c for complex.  Where np.longdouble is no wider than double, R_j of d / z is itself formed
  with an error of gamma_{K_j+64} G_j and the factor is (2 K_j + 130).  The bound of block j depends only on B and on
  blocks solved before it, so garbage cannot inflate its own bound and the first wrong block fails.  No element is left
  out of the comparison.

The CPU half (no GPU): a numpy emulation of the blocked algorithm in the working precision (block inverses, 64-column
steps, lower and upper) goes through the same checker: it must pass equality on every exact case, stay inside the bound
on every uniform case, and FAIL when one fault is injected: a 64-column block dropped from one Y_j, one element of one
W_j one ulp off (exact), one block solved with W_j where W_j^H is meant, one sentinel overwritten."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

TYPES = ["d", "z", "s", "c"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
LD_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
WIDE = {"s": np.float64, "c": np.complex128,
        "d": np.longdouble if LD_WIDER else np.float64, "z": np.clongdouble if LD_WIDER else np.complex128}
BITS = {"s": 24, "c": 24, "d": 53, "z": 53}
SENTINEL = {False: 1234.5, True: 1234.5 - 4321.25j}
W_SENTINEL = {False: -777.25, True: -777.25 + 55.5j}
JUNK = -9.9
JB = 64

DEFAULTS = dict(n=64, nb=64, nt=1, last_rows=None, pr=1, ri=0, il0=0, il1=1, ldb=None, gap=0, ldl=None, upper=0, unit=0,
                prio=0, info=0, offsets=(0, 0, 0), source="invert_diag_blocks", expect="strips")


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


def resolve(spec):
    s = dict(DEFAULTS, **spec)
    s["last_rows"] = s["last_rows"] or s["nb"]
    s["ldb"] = s["ldb"] or s["nb"]
    s["ldl"] = s["ldl"] or s["n"]
    ntl = s["il1"] - s["il0"]
    # a single tile may have b_ts = 0, as tile_trsm has it
    s["b_ts"] = 0 if (ntl == 1 and s["gap"] == 0) else s["ldb"] * s["n"] + s["gap"]
    return s


def extent(s, il):
    return s["last_rows"] if il * s["pr"] + s["ri"] == s["nt"] - 1 else s["nb"]


def mag(a):
    """|re| + |im|: what bounds the real products behind a complex one."""
    a = np.asarray(a)
    return (np.abs(a.real) + np.abs(a.imag)).astype(np.float64)


def unit_of(a):
    """The largest power of two that every entry of `a` (real and imaginary parts) is a whole multiple of."""
    v = np.concatenate([np.asarray(a).real.ravel(), np.asarray(a).imag.ravel()]).astype(np.float64)
    u = 1.0
    for _ in range(80):
        q = v / u
        if np.all(q == np.rint(q)):
            return u
        u /= 2
    raise AssertionError("entries are no multiples of a power of two")


@functools.lru_cache(maxsize=None)
def int_block(cx, index):
    """(N, M): N strictly LOWER triangular 64 x 64, sparse, small (Gaussian) integers; M = inv(I + N), an integer matrix
    with entries of magnitude <= 8.  The seed is searched for."""
    for seed in range(1000 * index, 1000 * index + 1000):
        rng = np.random.default_rng(seed)
        mask = np.tril(rng.random((JB, JB)) < (0.02 if cx else 0.03), -1)
        v = (rng.integers(1, 3, size=(JB, JB)) * rng.choice([-1, 1], size=(JB, JB))).astype(np.complex128)
        if cx:
            v = v + 1j * rng.integers(-1, 2, size=(JB, JB))
        n = np.where(mask, v, 0)
        a = np.eye(JB) + n
        inv = np.linalg.inv(a)
        m = np.rint(inv.real) + 1j * np.rint(inv.imag)
        if not (np.array_equal(a @ m, np.eye(JB)) and np.array_equal(m @ a, np.eye(JB))):
            continue
        if mag(m).max() <= 8 and np.count_nonzero(np.tril(m, -1)) >= 64:
            return (n, m) if cx else (n.real.copy(), m.real.copy())
    raise AssertionError("no seed gives a small integer inverse")


def draw(rng, shape, cx, kind):
    if kind == "exact":
        v = rng.integers(-8, 9, size=shape) / 8
        if cx:
            v = v + 1j * (rng.integers(-8, 9, size=shape) / 8)
    else:
        v = rng.uniform(-1, 1, size=shape) / 8
        if cx:
            v = v + 1j * rng.uniform(-1, 1, size=shape) / 8
    return v


def wide_solve(b, tri, upper, hp):
    """X with X tri^H = b, column by column in the type hp.  tri: the effective triangular matrix (n x n)."""
    n = tri.shape[0]
    x = np.zeros(b.shape, dtype=hp)
    t = tri.astype(hp)
    order = range(n - 1, -1, -1) if upper else range(n)
    for c in order:
        solved = slice(c + 1, n) if upper else slice(0, c)
        x[:, c] = (b[:, c].astype(hp) - x[:, solved] @ np.conj(t[c, solved])) / np.conj(t[c, c])
    return x


def wide_inverse(blk, upper, hp):
    """inv(blk) of a triangular block in the type hp, by substitution."""
    jb = blk.shape[0]
    eye = np.eye(jb, dtype=hp)
    # X blk = I  <=>  X (blk^H)^H = I: wide_solve with the adjoint, which is triangular the other way
    return wide_solve(eye, np.conj(blk.T), not upper, hp)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def reference(t, name, kind, seed=11):
    """Operands of one case and what the contract says comes out (cached: shared by the GPU test and the CPU check)."""
    s = resolve(ALL_CASES[name])
    cx = t in "cz"
    dt, hp = DT[t], WIDE[t]
    rng = np.random.default_rng(seed)
    n, ldl, upper, unit = s["n"], s["ldl"], s["upper"], s["unit"]
    nblk = -(-n // JB)
    # ---- the triangular matrix: `tri` is what the contract solves with, `lstore` what memory holds
    tri = np.zeros((n, n), dtype=dt)
    winv = np.zeros((nblk, JB, JB), dtype=hp)
    dense = draw(rng, (n, n), cx, kind).astype(dt)
    tri[:] = np.triu(dense) if upper else np.tril(dense)
    for j in range(nblk):
        j0, jb = j * JB, min(JB, n - j * JB)
        if kind == "exact":
            nn, mm = int_block(cx, j + (7 if upper else 0))
            if upper:
                nn, mm = nn.T, mm.T
            d1 = 2.0 ** rng.integers(-1, 2, size=JB)
            d2 = 1 / d1 if unit else 2.0 ** rng.integers(-1, 2, size=JB)
            blk = (d1[:, None] * (np.eye(JB) + nn) * d2[None, :])[:jb, :jb]
            wj = ((1 / d2)[:, None] * mm * (1 / d1)[None, :])[:jb, :jb]
        else:
            blk = tri[j0:j0 + jb, j0:j0 + jb].astype(np.complex128 if cx else np.float64)
            dg = rng.uniform(1, 2, size=jb) * rng.choice([-1, 1], size=jb)
            if cx:
                dg = dg * np.exp(2j * np.pi * rng.uniform(size=jb))
            blk[np.arange(jb), np.arange(jb)] = 1 if unit else dg
            blk = blk.astype(dt)
            wj = wide_inverse(blk, upper, hp)
        tri[j0:j0 + jb, j0:j0 + jb] = blk.astype(dt)
        winv[j, :jb, :jb] = wj
        assert np.array_equal(tri[j0:j0 + jb, j0:j0 + jb].astype(hp), np.asarray(blk).astype(hp))
    lstore = np.full((n, n), JUNK, dtype=dt)
    keep = np.triu(np.ones((n, n), dtype=bool)) if upper else np.tril(np.ones((n, n), dtype=bool))
    lstore[keep] = tri[keep]
    if unit:
        lstore[np.arange(n), np.arange(n)] = JUNK  # taken as 1, must not be read
    l_flat = np.full(ldl * n, JUNK, dtype=dt)
    l_flat.reshape(n, ldl).T[:n, :] = lstore
    winv_dt = winv.astype(dt)
    if kind == "exact":
        assert np.array_equal(winv_dt.astype(hp), winv), "the exact inverse is not representable"
        dg = np.abs(tri[np.arange(n), np.arange(n)])
        assert np.all(np.frexp(dg)[0] == 0.5) and np.all(tri[np.arange(n), np.arange(n)].imag == 0)

    # ---- B: tiles of [il0, il1) and one tile slot behind them that no launch may touch
    ntl = s["il1"] - s["il0"]
    ldb, b_ts = s["ldb"], s["b_ts"]
    slot = ldb * n + s["gap"]
    b0 = np.full((ntl + 1) * slot, SENTINEL[cx], dtype=dt)
    want = b0.copy()
    mask = np.zeros(b0.size, dtype=bool)
    tiles = []
    bits = 2.0 ** BITS[t]
    for il in range(s["il0"], s["il1"]):
        rows = extent(s, il)
        off = (il - s["il0"]) * b_ts
        view = lambda flat: flat[off:off + ldb * n].reshape(n, ldb).T[:rows, :]
        if kind == "exact":
            x = draw(rng, (rows, n), cx, kind).astype(dt)
            b = x.astype(hp) @ np.conj(tri.astype(hp)).T
            b_dt = b.astype(dt)
            assert np.array_equal(b_dt.astype(hp), b), "B is not representable"
            # every step exact in any order: sums of absolute values over the common unit
            ux, ul, uw = unit_of(x), unit_of(tri), unit_of(winv_dt)
            sums = mag(x) @ mag(tri).T
            assert 2 * sums.max() / (ux * ul) < bits, "B / Y_j"  # |B_j| + sum |X_p||L_jp| <= 2 sum |X||L|
            for j in range(nblk):
                cols = slice(j * JB, min(n, (j + 1) * JB))
                ljj = tri[cols, cols]
                wj = winv_dt[j][:ljj.shape[0], :ljj.shape[0]]
                y = x[:, cols].astype(hp) @ np.conj(ljj.astype(hp)).T
                assert (mag(y) @ mag(wj).T).max() / (ux * ul * uw) < bits, "Y_j W_j^H"
                p = mag(ljj) @ mag(wj)
                assert p.max() / (ul * uw) < bits and (mag(wj) @ p).max() / (uw * ul * uw) < bits, "inversion"
            xw = wide_solve(b, tri, upper, hp)
            assert np.array_equal(xw, x.astype(hp)), "the wide solve does not return the X the case was built from"
        else:
            b_dt = draw(rng, (rows, n), cx, "uniform").astype(dt) * 8
            x = None
        view(b0)[:] = b_dt
        view(mask)[:] = True
        if x is not None:
            view(want)[:] = x
        tiles.append((off, rows, b_dt))
    c = Case()
    c.s, c.t, c.kind, c.tri, c.l_flat, c.b0, c.want, c.mask, c.tiles = s, t, kind, tri, l_flat, b0, want, mask, tiles
    c.winv_hp, c.winv_dt, c.nblk = winv, winv_dt, nblk
    elem = np.dtype(dt).itemsize
    ob, ol, _ = s["offsets"]
    c.vec = all(v * elem % 16 == 0 for v in (ob, ldb, b_ts, ol, ldl))
    return c


def bits_differ(a, b):
    return ~(a.view(np.uint8).reshape(a.size, -1) == b.view(np.uint8).reshape(b.size, -1)).all(axis=1)


def check(c, got_b, got_w, path, vec, w_in):
    """The one checker: the GPU's result and the emulation's go through it.  Returns the largest residual / bound
    (uniform) or 0.0."""
    s, t, n = c.s, c.t, c.s["n"]
    cx, dt, hp = t in "cz", DT[t], WIDE[t]
    assert path == s["expect"], f"trsm_path chose {path}, the case is meant for {s['expect']}"
    if path == "strips":
        assert vec == c.vec, f"VEC = {vec}, the bases and strides say {c.vec}"
    if s["info"] != 0:
        assert not bits_differ(got_b, c.b0).any(), "B changed although *info != 0"
        assert not bits_differ(got_w, w_in).any(), "winv changed although *info != 0"
        return 0.0
    outside = np.flatnonzero(bits_differ(got_b, c.b0) & ~c.mask)
    assert outside.size == 0, (f"{outside.size} elements of B outside the contract changed; first: flat index "
                               f"{outside[0]}: {c.b0[outside[0]]} -> {got_b[outside[0]]}")
    # ---- winv as the device left it
    wblocks = got_w[:c.nblk * JB * JB].reshape(c.nblk, JB, JB).transpose(0, 2, 1)  # [block][row][col]
    if s["source"] == "caller":
        assert not bits_differ(got_w, w_in).any(), "the caller's winv changed"
    else:
        assert not bits_differ(got_w[c.nblk * JB * JB:], w_in[c.nblk * JB * JB:]).any(), "winv past the last block changed"
        if c.kind == "exact":
            bad = np.argwhere(wblocks != c.winv_dt)
            assert bad.size == 0, (f"{len(bad)} elements of winv differ from the exact inverse; first: block {bad[0][0]} "
                                   f"({bad[0][1]},{bad[0][2]}): got {wblocks[tuple(bad[0])]}, expected "
                                   f"{c.winv_dt[tuple(bad[0])]}")
    if c.kind == "exact":
        bad = np.flatnonzero((got_b != c.want) & c.mask)
        if bad.size:
            i = int(bad[0])
            til = i // s["b_ts"] if s["b_ts"] else 0
            col, row = divmod(i - til * s["b_ts"], s["ldb"])
            pytest.fail(f"{bad.size} of {int(c.mask.sum())} elements of X differ; first: tile {s['il0'] + til} row {row} "
                        f"(strip {row // 64}) column {col} (block column {col // 64}): got {got_b[i]}, expected {c.want[i]}")
        return 0.0
    # ---- uniform: component-wise residual bound, block column by block column
    u = np.finfo(dt).eps / 2
    wide = np.finfo(hp).eps < np.finfo(dt).eps
    worst = 0.0
    lw = c.tri.astype(hp)
    for off, rows, b_dt in c.tiles:
        xh = got_b[off:off + s["ldb"] * n].reshape(n, s["ldb"]).T[:rows, :]
        assert np.all(np.isfinite(xh)), "X is not finite"
        xw, bw = xh.astype(hp), b_dt.astype(hp)
        for j in range(c.nblk):
            cols = slice(j * JB, min(n, (j + 1) * JB))
            solved = slice(cols.stop, n) if s["upper"] else slice(0, cols.start)
            kj = solved.stop - solved.start
            jb = cols.stop - cols.start
            r = bw[:, cols] - xw[:, solved] @ np.conj(lw[cols, solved]).T - xw[:, cols] @ np.conj(lw[cols, cols]).T
            g = np.abs(b_dt[:, cols]).astype(np.float64) + \
                np.abs(xh[:, solved]).astype(np.float64) @ np.abs(c.tri[cols, solved]).astype(np.float64).T
            wl = np.abs(c.winv_hp[j][:jb, :jb]).astype(np.float64).T @ np.abs(c.tri[cols, cols]).astype(np.float64).T
            factor = (kj + 66) if wide else (2 * kj + 130)
            bound = (4 if cx else 1) * factor * u * (g @ wl)
            ratio = np.abs(r).astype(np.float64) / bound
            if not ratio.max() <= 1.0:
                rr, cc = np.unravel_index(np.nanargmax(ratio), ratio.shape)
                pytest.fail(f"tile at {off} row {rr} (strip {rr // 64}) block column {j} column {cc}: |residual| = "
                            f"{abs(r[rr, cc]):.3e} is {ratio[rr, cc]:.2f} x the bound {bound[rr, cc]:.3e}")
            worst = max(worst, float(ratio.max()))
    return worst


def winv_input(c):
    """What the winv buffer holds before the launch: the caller's inverse, or a sentinel the device writes over; one
    more block of sentinel behind the last one in both cases."""
    dt = DT[c.t]
    w = np.full((c.nblk + 1) * JB * JB, W_SENTINEL[c.t in "cz"], dtype=dt)
    if c.s["source"] == "caller":
        w[:c.nblk * JB * JB] = c.winv_dt.transpose(0, 2, 1).ravel()
    return w


def run_case(dlaf, t, name, kind="exact"):
    c = reference(t, name, kind)
    s = c.s
    got_b, w_in = c.b0.copy(), winv_input(c)
    got_w = w_in.copy()
    fields = {k: s[k] for k in ("b_ts", "ldb", "il0", "il1", "pr", "ri", "nb", "nt", "last_rows", "ldl", "n", "upper",
                                "prio", "info", "unit")}
    path, vec, info = dlaf.trsm_direct(got_b, c.l_flat, got_w, winv_source=s["source"], offsets=s["offsets"], **fields)
    assert info == s["info"], f"*info came back as {info}"
    worst = check(c, got_b, got_w, path, vec, w_in)
    if kind == "uniform":
        print(f"{name}, {t}: max |residual| / bound = {worst:.3f}")
    return worst


def emulate(c, fault=None):
    """The blocked algorithm in the working precision: block inverses, 64-column steps.  Returns (B buffer, winv buffer)
    as a launch would leave them.  fault: None, 'drop', 'ulp', 'transposed' or 'sentinel'."""
    s, n, dt = c.s, c.s["n"], DT[c.t]
    w_in = winv_input(c)
    got_w = w_in.copy()
    got_b = c.b0.copy()
    if s["info"] != 0:
        return got_b, got_w, w_in
    wd = c.winv_dt.copy()
    order = list(range(c.nblk - 1, -1, -1) if s["upper"] else range(c.nblk))
    # the block a fault goes into: the last full one solved
    jf = next(j for j in reversed(order) if min(n, (j + 1) * JB) - j * JB == JB) if n >= JB else order[-1]
    if fault == "ulp":
        real = wd.real.dtype.type
        v = wd[jf, 0, 0]
        wd[jf, 0, 0] = np.nextafter(real(v.real), real(np.inf)) + (1j * v.imag if c.t in "cz" else 0)
    if s["source"] != "caller":
        got_w[:c.nblk * JB * JB] = wd.transpose(0, 2, 1).ravel()
    for off, rows, b_dt in c.tiles:
        x = b_dt.copy()
        for j in order:
            cols = slice(j * JB, min(n, (j + 1) * JB))
            solved = slice(cols.stop, n) if s["upper"] else slice(0, cols.start)
            if fault == "drop" and j == jf:
                assert solved.stop - solved.start >= JB, "the case has no solved block to drop"
                solved = slice(solved.start + JB, solved.stop) if s["upper"] else slice(solved.start, solved.stop - JB)
            jb = cols.stop - cols.start
            y = x[:, cols] - x[:, solved] @ np.conj(c.tri[cols, solved]).T
            wj = wd[j][:jb, :jb]
            x[:, cols] = y @ (wj if (fault == "transposed" and j == jf) else np.conj(wj).T)
            assert x.dtype == dt
        got_b[off:off + s["ldb"] * n].reshape(n, s["ldb"]).T[:rows, :] = x
    if fault == "sentinel":
        free = np.flatnonzero(~c.mask)
        got_b[free[len(free) // 2]] = 0
    return got_b, got_w, w_in


# ---- the cases -----------------------------------------------------------------------------------------------------
def single(n, nb, **kw):
    return dict(n=n, nb=nb, **kw)


def panel(n, nb, last_rows=64, **kw):
    """Local tiles 1 and 2 of process row 1 of 2: global tiles 3 and 5 = nt - 1, the last one ragged; padded B
    (ldb = nb + 2), a gap between the tiles, padded L (ldl = n + 2)."""
    return dict(dict(n=n, nb=nb, il0=1, il1=3, pr=2, ri=1, nt=6, last_rows=last_rows, ldb=nb + 2, gap=4, ldl=n + 2), **kw)


ROWS_D = {}
for _n, _path in ((256, "rows-256"), (512, "rows-256"), (768, "rows-256"), (128, "rows-128"), (384, "rows-128")):
    ROWS_D[f"{_path} n={_n} nb=64 one tile"] = single(_n, 64, expect=_path)
    ROWS_D[f"{_path} n={_n} nb=128 panel ragged last tile prio"] = panel(_n, 128, prio=1, expect=_path)
    ROWS_D[f"{_path} n={_n} nb=192 panel potrf_diag"] = panel(_n, 192, source="potrf_diag", expect=_path)
ROWS_Z = {}
for _n in (128, 256, 384):
    ROWS_Z[f"rows-z n={_n} nb=64 one tile"] = single(_n, 64, expect="rows-z")
    ROWS_Z[f"rows-z n={_n} nb=128 panel ragged last tile prio"] = panel(_n, 128, prio=1, expect="rows-z")
    ROWS_Z[f"rows-z n={_n} nb=192 panel potrf_diag"] = panel(_n, 192, source="potrf_diag", expect="rows-z")

# each of these must report strips and still be equal (d and z)
EDGES = {
    "edge last_rows=65": panel(256, 128, last_rows=65),
    "edge n=320": panel(320, 128),
    "edge odd ldb": panel(256, 128, ldb=129),
    "edge B base off by one element": panel(256, 128, offsets=(1, 0, 0)),
    "edge L base off by one element": panel(256, 128, offsets=(0, 1, 0)),
    "edge upper n=256": panel(256, 128, upper=1),
}

# a complex double element is 16 bytes: odd strides and one-element offsets stay aligned, those edges are d only
Z_EDGES = ("edge last_rows=65", "edge n=320", "edge upper n=256")

STRIPS = {}
for _i, _n in enumerate((1, 17, 64, 65, 130, 192)):
    for _k, _nb in enumerate((64, 128, 200)):
        for _up in (0, 1):
            if (_i + _k) % 2:  # odd strides: the non-VEC loaders for s, d and c
                STRIPS[f"strips n={_n} nb={_nb} upper={_up} odd ld"] = single(_n, _nb, upper=_up, ldb=_nb + 1, ldl=_n + 1 + _n % 2)
            else:              # multiples of four with padding: VEC for every type
                STRIPS[f"strips n={_n} nb={_nb} upper={_up} padded ld"] = single(_n, _nb, upper=_up, ldb=_nb + 8 - _nb % 4,
                                                                             ldl=_n + 8 - _n % 4)
for _nb in (64, 128, 200):
    for _up in (0, 1):
        # global tiles 2, 5, 8 = nt - 1 on process row 2 of 3, the last with 37 rows
        STRIPS[f"strips panel n=130 nb={_nb} upper={_up} last_rows=37"] = dict(
            n=130, nb=_nb, upper=_up, il0=0, il1=3, pr=3, ri=2, nt=9, last_rows=37, ldb=_nb + 4, gap=8, ldl=136)

INVERT = {}
for _kb in (1, 17, 64, 65, 130):
    for _up in (0, 1):
        for _unit in (0, 1):
            for _src in ("invert_diag_blocks", "potrf_diag"):
                INVERT[f"{_src} kb={_kb} upper={_up} unit={_unit}"] = single(_kb, 64, upper=_up, unit=_unit, source=_src,
                                                                            ldl=_kb + 3)

INFO = {
    "info!=0 strips": dict(single(130, 128, ldl=132), info=7),
    "info!=0 rows-256": dict(panel(256, 128), info=-3, expect="rows-256"),
    "info!=0 rows-z": dict(panel(256, 128), info=-3, expect="rows-z"),
}

UNIFORM_ROWS = {
    "uniform rows-256 n=512": dict(panel(512, 128, prio=1), source="caller", expect="rows-256"),
    "uniform rows-128 n=384": dict(panel(384, 128), source="caller", expect="rows-128"),
    "uniform rows-z n=384": dict(panel(384, 128), source="caller", expect="rows-z"),
}
UNIFORM_STRIPS = {
    "uniform strips n=130 lower": dict(n=130, nb=200, ldb=204, ldl=136, source="caller"),
    "uniform strips n=130 upper": dict(n=130, nb=200, ldb=204, ldl=136, upper=1, source="caller"),
}
ALL_CASES = {**ROWS_D, **ROWS_Z, **EDGES, **STRIPS, **INVERT, **INFO, **UNIFORM_ROWS, **UNIFORM_STRIPS}
# the strips switch: the row-owner shapes again, in a child process
SWITCHED = {f"switched {k}": dict(v, expect="strips") for k, v in {**ROWS_D, **ROWS_Z}.items() if "nb=192" not in k}
ALL_CASES.update(SWITCHED)


EXACT = ([("d", k) for k in ROWS_D] + [("z", k) for k in ROWS_Z] + [(t, k) for k in EDGES for t in "dz" if t == "d" or k in Z_EDGES] +
         [(t, k) for k in STRIPS for t in TYPES] + [(t, k) for k in INVERT for t in TYPES] +
         [(t, "info!=0 strips") for t in TYPES] + [("d", "info!=0 rows-256"), ("z", "info!=0 rows-z")])
UNIFORM = ([("d", "uniform rows-256 n=512"), ("d", "uniform rows-128 n=384"), ("z", "uniform rows-z n=384")] +
           [(t, k) for k in UNIFORM_STRIPS for t in TYPES])
SWITCHED_TYPED = [("z" if "rows-z" in k else "d", k) for k in SWITCHED]


def ids(pairs):
    return [pytest.param(t, k, id=f"{k}, {t}") for t, k in pairs]


@gpu
@pytest.mark.parametrize("t,name", ids(EXACT))
def test_trsm_exact(dlaf, t, name):
    run_case(dlaf, t, name)


@gpu
@pytest.mark.parametrize("t,name", ids(UNIFORM))
def test_trsm_uniform_componentwise_bound(dlaf, t, name):
    run_case(dlaf, t, name, kind="uniform")


def test_row_owner_cases_are_wellformed():
    """No GPU: the row-owner cases satisfy what trsm_path asks of a launch (the GPU test asserts the reported path; a
    typo in a case fails here already)."""
    for t, k in EXACT + UNIFORM:
        s = resolve(ALL_CASES[k])
        if k.startswith(("rows", "uniform rows")):
            macro = 256 if s["expect"] == "rows-256" else 128
            assert s["n"] % macro == 0 and s["nb"] % 64 == 0 and s["last_rows"] % 64 == 0 and not s["upper"], k
            elem = np.dtype(DT[t]).itemsize
            assert all(v * elem % 16 == 0 for v in (s["ldb"], s["b_ts"], s["ldl"])), k


def test_emulation_passes_every_case_and_faults_fail():
    """No GPU.  The working-precision emulation of the blocked algorithm through the checker the GPU results go
    through: equality on every exact case, inside the bound on every uniform case, and a failure for every injected
    fault.  Prints the largest residual / bound of the emulation."""
    for t, k in EXACT + SWITCHED_TYPED:
        c = reference(t, k, "exact")
        got_b, got_w, w_in = emulate(c)
        check(c, got_b, got_w, c.s["expect"], c.vec, w_in)
    worst = 0.0
    for t, k in UNIFORM:
        c = reference(t, k, "uniform")
        got_b, got_w, w_in = emulate(c)
        worst = max(worst, check(c, got_b, got_w, c.s["expect"], c.vec, w_in))
    print(f"emulation: max |residual| / bound over the uniform cases = {worst:.3f}")
    assert 0 < worst <= 1
    # injected faults, on one case per path (exact and uniform) and on strips lower / upper of every type
    targets = [("d", "rows-256 n=512 nb=128 panel ragged last tile prio", "exact"),
               ("d", "rows-128 n=384 nb=128 panel ragged last tile prio", "exact"),
               ("z", "rows-z n=384 nb=128 panel ragged last tile prio", "exact")]
    targets += [(t, f"strips panel n=130 nb=128 upper={up} last_rows=37", "exact") for t in TYPES for up in (0, 1)]
    targets += [(t, k, "uniform") for t, k in UNIFORM]
    for t, k, kind in targets:
        c = reference(t, k, kind)
        for fault in ("drop", "ulp", "transposed", "sentinel"):
            if fault == "ulp" and kind != "exact":
                continue
            got_b, got_w, w_in = emulate(c, fault)
            with pytest.raises(BaseException) as e:
                check(c, got_b, got_w, c.s["expect"], c.vec, w_in)
            assert isinstance(e.value, (AssertionError, pytest.fail.Exception)), (t, k, kind, fault, e.value)
    # a wrong path is a failure too
    c = reference("d", "rows-256 n=256 nb=64 one tile", "exact")
    got_b, got_w, w_in = emulate(c)
    with pytest.raises(AssertionError):
        check(c, got_b, got_w, "strips", c.vec, w_in)


SWITCH_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import dla_future_amd as dl
import test_gpu_trsm_kernel as m
dl.initialize()
failed = 0
for t, name in m.SWITCHED_TYPED:
    try:
        m.run_case(dl, t, name)
    except BaseException as e:
        failed += 1
        print("FAILED:", name + ",", t, "--", str(e)[:600], flush=True)
print("DONE", len(m.SWITCHED_TYPED), failed, flush=True)
"""


@gpu
def test_trsm_strips_switch_exact():
    """DLAF_MI355X_TRSM=strips is read once per process: one child process runs the rows-256, rows-128 and rows-z
    shapes, which must report strips and give the same bits as the reference."""
    r = subprocess.run([sys.executable, "-c", SWITCH_CHILD % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT,
                       env=dict(os.environ, DLAF_MI355X_TRSM="strips"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and f"DONE {len(SWITCHED_TYPED)} 0" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


@gpu
def test_trsm_direct_refuses_out_of_bounds(dlaf):
    """The entry launches nothing when a field would make a kernel touch memory outside an operand."""
    c = reference("d", "rows-256 n=256 nb=128 panel ragged last tile prio", "exact")
    s = c.s
    base = {k: s[k] for k in ("b_ts", "ldb", "il0", "il1", "pr", "ri", "nb", "nt", "last_rows", "ldl", "n", "upper",
                              "prio", "info", "unit")}
    w = winv_input(c)
    for change in (dict(il1=4), dict(n=257), dict(nt=5), dict(ldb=127), dict(ldl=255), dict(b_ts=s["b_ts"] * 3),
                   dict(last_rows=129), dict(ri=2)):
        b = c.b0.copy()
        with pytest.raises(ValueError):
            dlaf.trsm_direct(b, c.l_flat, w.copy(), **dict(base, **change))
        assert not bits_differ(b, c.b0).any()
    with pytest.raises(ValueError):
        dlaf.trsm_direct(c.b0.copy(), c.l_flat, w[:JB * JB].copy(), **base)      # winv too short
    with pytest.raises(ValueError):
        dlaf.trsm_direct(c.b0.copy(), c.l_flat, w.copy(), offsets=(0, 0, 1), **base)  # winv off 16-byte alignment
