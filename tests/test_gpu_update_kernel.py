"""The grouped update kernel (launch_update, csrc/device/kernels_update.hip) called directly, one launch per case,
through dlaf.update_direct, against a plain numpy reference looped tile by tile over GLOBAL tile indices.  The
reference is written from the kernel's contract (the comments of csrc/device/device_api.hpp), not from the kernel.

Two kinds of operands, neither with a measured tolerance:

* exact: entries of A, B (and C for d / z) are multiples of 2^-6 in [-1, 1]; for s / c A and B are multiples of 2^-3
  and C of 2^-6.  With K <= 512 every product and every partial sum, in any order, is exactly representable, so the
  assertion is equality of every element the contract says is updated -- whatever summation order K-phase alignment or
  work stealing produce.  reference() asserts that the sum in the working precision equals the one in the wider type.
* uniform(-1, 1): |got - ref| <= c (K + 2) u (|C0| + |A| |B|^H) component-wise, u the unit roundoff, ref in float64
  for s / c and in np.longdouble for d / z, c = 1 real / 4 complex (inner-product bound and the complex-multiply
  constant).  Where np.longdouble is no wider than double the reference of d / z is float64 and the factor (K + 3).

Every element of the C buffer outside the contract (tiles above the diagonal, the strict upper half of diagonal tiles,
rows / columns past a ragged extent, the padding between nb and ldc, tiles outside the launch's range) holds a sentinel
and must come back bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

TYPES = ["d", "z", "s", "c"]
DT = {"s": np.float32, "d": np.float64, "c": np.complex64, "z": np.complex128}
BLK = {"s": (128, 128, 16), "d": (128, 128, 16), "c": (128, 128, 16), "z": (128, 64, 8)}  # BM, BN, BK of UpdateCfg<T>
LD_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
SENTINEL = {False: 1234.5, True: 1234.5 - 4321.25j}

DEFAULTS = dict(nb=128, ldc=None, ld=None, pr=1, pc=1, ri=0, ci=0, nt=3, last_rows=None, rect=0, nt_c=0, last_cols=0,
                il0=0, il1=None, jl0=0, jl1=None, K="BK", K1=0, her2k=0, b_period=1, b_jl0=-1, role=2, max_blocks=0,
                excl_rounds=0, info=0, offsets=(0, 0, 0, 0, 0), tile_layout=False, repeat=False, expect=None)


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


def resolve(t, spec):
    """DEFAULTS + spec with everything that depends on the type (BK) or on other fields worked out."""
    s = dict(DEFAULTS, **spec)
    bk = BLK[t][2]
    if isinstance(s["K1"], str):
        s["K1"] = int(eval(s["K1"], {"BK": bk}))
    if isinstance(s["K"], str):
        s["K"] = int(eval(s["K"], {"BK": bk, "K1": s["K1"]}))
    s["ldc"] = s["ldc"] or s["nb"]
    s["ld"] = s["ld"] or s["nb"]
    s["last_rows"] = s["last_rows"] or s["nb"]
    ntc = s["nt_c"] if s["rect"] else s["nt"]
    s["ltr"] = -(-(s["nt"] - s["ri"]) // s["pr"])
    s["ltc"] = -(-(ntc - s["ci"]) // s["pc"])
    s["il1"] = s["ltr"] if s["il1"] is None else s["il1"]
    s["jl1"] = s["ltc"] if s["jl1"] is None else s["jl1"]
    return s


def draw(rng, shape, t, kind, denom):
    cx = t in "cz"
    if kind == "exact":
        v = rng.integers(-denom, denom + 1, size=shape) / denom
        if cx:
            v = v + 1j * (rng.integers(-denom, denom + 1, size=shape) / denom)
    else:
        v = rng.uniform(-1, 1, size=shape)
        if cx:
            v = v + 1j * rng.uniform(-1, 1, size=shape)
    return v.astype(DT[t])


def extent(g, nt, last, nb):
    return last if g == nt - 1 else nb


def reference(t, s, kind, rng, wide_exact=False):
    """Operands of one launch and what the contract says comes out.  Returns the flat host arrays (c0, a, b, a2, b2),
    the expected flat C, the mask of elements the contract updates, and the flat bound (None for exact operands)."""
    cx = t in "cz"
    dt = DT[t]
    nb, ldc, ld, K, K1 = s["nb"], s["ldc"], s["ld"], s["K"], s["K1"]
    k1 = K1 if K1 > 0 else K
    k2 = K - k1
    kp = max(k1, k2)  # columns every panel tile holds
    il0, il1, jl0, jl1 = s["il0"], s["il1"], s["jl0"], s["jl1"]
    bj0 = s["b_jl0"] if s["b_jl0"] >= 0 else jl0
    per = s["b_period"]
    if s["tile_layout"]:
        assert ldc == nb and ld == nb and kp <= nb
        tile_a = nb * nb
    else:
        tile_a = ld * kp
    c_tsr = ldc * nb
    c_tsc = c_tsr * s["ltr"]
    denom_ab = 64 if t in "dz" else 8
    sent = dt(SENTINEL[cx])

    def panel(ntiles):
        flat = np.full(ntiles * tile_a, sent, dtype=dt)
        tiles = [flat[i * tile_a:i * tile_a + ld * kp].reshape(kp, ld).T for i in range(ntiles)]  # [row, k] views
        return flat, tiles

    a_flat, a_t = panel(il1 - il0)
    a2_flat, a2_t = panel(il1 - il0) if K1 > 0 else (None, None)
    nbt = jl1 - bj0
    groups = -(-nbt // per)
    b_ts, b_ts2 = tile_a, groups * tile_a
    b_flat, b_all = panel(groups * per)
    b2_flat, b2_all = panel(groups * per) if K1 > 0 else (None, None)

    def b_tile(tiles, jl):
        jt = jl - bj0
        return tiles[(jt % per) * groups + jt // per]

    ntc = s["nt_c"] if s["rect"] else s["nt"]
    lastc = s["last_cols"] if s["rect"] else s["last_rows"]
    for il in range(il0, il1):
        rows = extent(il * s["pr"] + s["ri"], s["nt"], s["last_rows"], nb)
        a_t[il - il0][:rows, :] = draw(rng, (rows, kp), t, kind, denom_ab)
        if K1 > 0:
            a2_t[il - il0][:rows, :] = draw(rng, (rows, kp), t, kind, denom_ab)
    for jl in range(bj0, jl1):
        cols = extent(jl * s["pc"] + s["ci"], ntc, lastc, nb)
        b_tile(b_all, jl)[:cols, :] = draw(rng, (cols, kp), t, kind, denom_ab)
        if K1 > 0:
            b_tile(b2_all, jl)[:cols, :] = draw(rng, (cols, kp), t, kind, denom_ab)

    c0 = np.full(c_tsc * s["ltc"], sent, dtype=dt)
    want = c0.copy()
    mask = np.zeros(c0.size, dtype=bool)
    bound = None if kind == "exact" else np.zeros(c0.size, dtype=np.float64)

    def c_view(flat, il, jl):
        off = il * c_tsr + jl * c_tsc
        return flat[off:off + ldc * nb].reshape(nb, ldc).T  # [row, col], rows up to ldc

    if kind == "exact":
        # float64 is exact for these operands; wide_exact (the CPU check) puts d / z against np.longdouble as well
        hp = (np.clongdouble if cx else np.longdouble) if (wide_exact and t in "dz") else (np.complex128 if cx else np.float64)
    elif t in "dz":
        hp = (np.clongdouble if cx else np.longdouble) if LD_WIDER else (np.complex128 if cx else np.float64)
    else:
        hp = np.complex128 if cx else np.float64
    sign = 1 if s["role"] == 4 else -1
    for il in range(il0, il1):
        gi = il * s["pr"] + s["ri"]
        rows = extent(gi, s["nt"], s["last_rows"], nb)
        for jl in range(jl0, jl1):
            gj = jl * s["pc"] + s["ci"]
            if not s["rect"] and gi < gj:
                continue
            cols = extent(gj, ntc, lastc, nb)
            diag = (not s["rect"]) and gi == gj
            row1 = a_t[il - il0][:rows, :k1]
            row2 = a2_t[il - il0][:rows, :k2] if k2 else None
            if not diag:
                col1 = b_tile(b_all, jl)[:cols, :k1]
                col2 = b_tile(b2_all, jl)[:cols, :k2] if k2 else None
            elif not s["her2k"]:
                col1 = a_t[il - il0][:cols, :k1]  # the column operand of a diagonal tile is the row panel's tile
                col2 = a2_t[il - il0][:cols, :k2] if k2 else None
            else:
                col1 = a2_t[il - il0][:cols, :k1]  # her2k: the row panel again, segments swapped
                col2 = a_t[il - il0][:cols, :k2]
            cv = draw(rng, (rows, cols), t, kind, 64)

            def product(ty, absolute=False):
                f = (lambda x: np.abs(x).astype(np.float64)) if absolute else (lambda x: x.astype(ty))
                p = f(row1) @ f(col1).conj().T
                if k2:
                    p = p + f(row2) @ f(col2).conj().T
                return p

            new_hp = cv.astype(hp) + sign * product(hp)
            if kind == "exact" and np.dtype(hp) != np.dtype(dt):
                new_wp = cv + sign * product(dt)
                assert new_wp.dtype == dt and np.array_equal(new_wp.astype(hp), new_hp), \
                    "operands are not exact in the working precision"
            new = new_hp.astype(dt)
            upd = np.ones((rows, cols), dtype=bool)
            if diag:
                upd = np.tril(upd)
                if cx:
                    idx = np.arange(rows)
                    new[idx, idx] = new[idx, idx].real
            c_view(c0, il, jl)[:rows, :cols][upd] = cv[upd]
            c_view(want, il, jl)[:rows, :cols][upd] = new[upd]
            c_view(mask, il, jl)[:rows, :cols][upd] = True
            if bound is not None:
                u = np.finfo(dt).eps / 2
                kf = K + 2 if (LD_WIDER or t in "sc") else K + 3
                bnd = (4 if cx else 1) * kf * u * (np.abs(cv).astype(np.float64) + product(None, absolute=True))
                c_view(bound, il, jl)[:rows, :cols][upd] = bnd[upd]
                # the reference at full width, for the comparison (want holds it rounded to the working type)
                s.setdefault("_hp", {})[(il, jl)] = (new_hp, upd)
    geo = dict(c_tsr=c_tsr, c_tsc=c_tsc, ldc=ldc, a_ts=tile_a, lda=ld, ldb=ld, b_ts=b_ts, b_ts2=b_ts2)
    return (c0, a_flat, b_flat, a2_flat, b2_flat), want, mask, bound, geo


def where(s, geo, flat_index):
    jl, rem = divmod(int(flat_index), geo["c_tsc"])
    il, rem = divmod(rem, geo["c_tsr"])
    col, row = divmod(rem, geo["ldc"])
    return (f"local tile ({il},{jl}) = global ({il * s['pr'] + s['ri']},{jl * s['pc'] + s['ci']}), "
            f"element ({row},{col})")


def run_case(dlaf, t, spec, kind="exact", seed=7):
    s = resolve(t, spec)
    rng = np.random.default_rng(seed)
    (c0, a, b, a2, b2), want, mask, bound, geo = reference(t, s, kind, rng)
    fields = {k: s[k] for k in ("il0", "il1", "jl0", "jl1", "nb", "K", "pr", "ri", "pc", "ci", "nt", "last_rows", "rect",
                                "nt_c", "last_cols", "K1", "her2k", "b_period", "b_jl0", "info", "role", "max_blocks",
                                "excl_rounds", "ltr", "ltc")}
    fields.update(tile_layout=int(s["tile_layout"]), b_ts=geo["b_ts"], b_ts2=geo["b_ts2"])
    if not s["tile_layout"]:
        fields.update({k: geo[k] for k in ("c_tsr", "c_tsc", "ldc", "a_ts", "lda", "ldb")})
    got = c0.copy()
    persistent, exclusive, again = dlaf.update_direct(got, a, b, a2=a2, b2=b2, offsets=s["offsets"], repeat=s["repeat"],
                                                      **fields)
    launches = 2 if s["repeat"] else 1
    if s["expect"] == "plain":
        assert persistent == 0, "the launch took the persistent form"
    elif s["expect"] == "persistent":
        assert (persistent, exclusive) == (launches, 0), (persistent, exclusive)
    elif s["expect"] == "exclusive":
        assert (persistent, exclusive) == (launches, launches), (persistent, exclusive)
    if s["info"] != 0:
        want, mask = c0, np.zeros_like(mask)
    for res, label in [(got, "")] + ([(again, " (repeated launch)")] if s["repeat"] else []):
        same = res.view(np.uint8).reshape(res.size, -1) == want.view(np.uint8).reshape(want.size, -1)
        outside = np.flatnonzero(~same.all(axis=1) & ~mask)
        assert outside.size == 0, (f"{outside.size} elements outside the contract changed{label}; first: "
                                   f"{where(s, geo, outside[0])}: {c0[outside[0]]} -> {res[outside[0]]}")
        if kind == "exact" or s["info"] != 0:
            bad = np.flatnonzero((res != want) & mask)
            assert bad.size == 0, (f"{bad.size} of {int(mask.sum())} updated elements differ{label}; first: "
                                   f"{where(s, geo, bad[0])}: got {res[bad[0]]}, expected {want[bad[0]]}")
        else:
            worst = 0.0
            for (il, jl), (new_hp, upd) in s["_hp"].items():
                off = il * geo["c_tsr"] + jl * geo["c_tsc"]
                view = lambda flat: flat[off:off + geo["ldc"] * s["nb"]].reshape(s["nb"], geo["ldc"]).T[
                    :new_hp.shape[0], :new_hp.shape[1]]
                g_hp = view(res).astype(new_hp.dtype)
                if t in "cz":
                    idx = np.arange(min(new_hp.shape))
                    if (not s["rect"]) and il * s["pr"] + s["ri"] == jl * s["pc"] + s["ci"]:
                        assert np.all(view(res)[idx, idx].imag == 0), f"diagonal of tile ({il},{jl}) is not real"
                        new_hp = new_hp.copy()
                        new_hp[idx, idx] = new_hp[idx, idx].real
                err = np.abs(g_hp - new_hp).astype(np.float64)
                bnd = view(bound)
                ratio = np.where(upd, err / np.where(bnd > 0, bnd, 1.0), 0.0)
                assert not np.any(upd & (bnd <= 0) & (err > 0))
                if ratio.max() > 1.0:
                    r, c = np.unravel_index(np.argmax(ratio), ratio.shape)
                    pytest.fail(f"tile ({il},{jl}) element ({r},{c}): |got - ref| = {err[r, c]:.3e} is "
                                f"{ratio[r, c]:.2f} x the bound {bnd[r, c]:.3e}{label}")
                worst = max(worst, float(ratio.max()))
            print(f"{t}: max |got - ref| / bound = {worst:.3f}")


# ---- the cases -----------------------------------------------------------------------------------------------------
SMALL = dict(nb=192, nt=3, last_rows=37)  # fewer than 16 block rows: no patches, no XCD remap; ragged blocks
PLAIN = {
    # tile shape
    "nb=128 tile-layout": dict(nb=128, tile_layout=True, last_rows=37, expect="plain"),
    "nb=192 ragged-block-in-every-tile": dict(nb=192, tile_layout=True, expect="plain"),
    "nb=256": dict(nb=256, tile_layout=True, K="4*BK"),
    "nb=129 ldc=129 non-VEC": dict(nb=129, last_rows=1),
    "nb=128 ldc=136 ld=130 padding": dict(nb=128, ldc=136, ld=130, last_rows=37),
    "nb=128 unaligned device bases": dict(nb=128, nt=3, offsets=(1, 1, 1, 0, 0)),
    "nb=128 unaligned a2 b2 bases": dict(nb=128, nt=3, K1="BK", K="2*K1", offsets=(0, 0, 0, 1, 1)),
    "last_rows=1": dict(nb=192, last_rows=1),
    "last_rows=37": dict(nb=192, last_rows=37),
    "last_rows=nb": dict(nb=192, last_rows=192),
    # map
    "map 17 block rows": dict(nt=17, tile_layout=True),
    "map 25 block rows ragged last patch": dict(nt=25, last_rows=37, tile_layout=True),
    "map 17 block rows ld=129 ldc=129": dict(nt=17, ldc=129, ld=129, last_rows=37),
    "map il0>0": dict(nt=17, il0=3, tile_layout=True),
    "map single column jl0=5 role=1": dict(nt=17, il0=5, jl0=5, jl1=6, role=1, tile_layout=True),
    "map nb=256 single column jl0=3 role=1": dict(nb=256, nt=9, il0=3, jl0=3, jl1=4, role=1, last_rows=37),
    "map column range starting below il0": dict(nt=25, il0=2, jl0=10, last_rows=37, tile_layout=True),
    # rectangular form
    "rect wide nt=2 nt_c=5": dict(nb=192, rect=1, nt=2, nt_c=5, last_rows=37, last_cols=100, role=3, tile_layout=True),
    "rect tall nt=5 nt_c=2": dict(nb=192, rect=1, nt=5, nt_c=2, last_rows=100, last_cols=37, role=3, tile_layout=True),
    "rect patches nt=17 nt_c=37 pc=2 ci=1": dict(rect=1, nt=17, nt_c=37, pc=2, ci=1, last_rows=37, last_cols=5, role=3,
                                                 tile_layout=True),
    "rect role=4 adds": dict(nb=192, rect=1, nt=3, nt_c=2, last_rows=37, last_cols=192, role=4, K=40),
    # K
    "K=2BK": dict(SMALL, K="2*BK"),
    "K=40": dict(SMALL, K=40),
    "K=7": dict(SMALL, K=7),
    "K=512": dict(nb=256, nt=3, last_rows=37, K=512),
    # panel layout
    "b_period=2 b_jl0<jl0 column sub-range": dict(nt=9, jl0=2, jl1=7, b_jl0=1, b_period=2, last_rows=37),
    "b_period=3 b_jl0<jl0 column sub-range": dict(nt=9, il0=1, jl0=3, jl1=8, b_jl0=1, b_period=3, K=40),
    "b_period=3 patches": dict(nt=20, jl0=1, b_jl0=0, b_period=3, last_rows=37),
    # info
    "info!=0 plain": dict(SMALL, info=3),
}
for _k1 in ("BK", "3*BK", "24", "5"):
    for _k in ("2*K1", "K1+7"):
        PLAIN[f"two-segment K1={_k1} K={_k}"] = dict(SMALL, K1=_k1, K=_k)
        PLAIN[f"her2k K1={_k1} K={_k} ragged last diagonal tile"] = dict(SMALL, K1=_k1, K=_k, her2k=1, role=3)
PLAIN["two-segment full blocks K1=3BK K=6BK nb=256"] = dict(nb=256, nt=3, K1="3*BK", K="2*K1")
PLAIN["her2k full blocks K1=2BK K=4BK nb=256"] = dict(nb=256, nt=3, K1="2*BK", K="2*K1", her2k=1, role=3)
for _r in range(5):
    # nb = 256: interior blocks, so roles 1 to 3 of d take the "C preloaded into the accumulators" path
    PLAIN[f"role={_r} plain"] = dict(nb=256, nt=3, last_rows=37, role=_r, K="4*BK", expect="plain")

# at least 384 work items: 17 block rows, 6 patches of 64 (z: 128)
BULK = dict(nt=17, last_rows=37, max_blocks=16, expect="persistent")
PERSISTENT = {
    "persistent max_blocks=8 role=0 UTAIL": dict(BULK, max_blocks=8, role=0, K="8*BK", tile_layout=True),
    "persistent max_blocks=16 role=0 UTAIL": dict(BULK, max_blocks=16, role=0, K="8*BK"),
    "persistent max_blocks=20 role=0 UTAIL K=BK 25 block rows": dict(BULK, nt=25, max_blocks=20, role=0),
    "persistent role=0 two-segment K1=3BK K=6BK": dict(BULK, role=0, K1="3*BK", K="2*K1"),
    "persistent role=0 two-segment K1=24 K=31": dict(BULK, role=0, K1=24, K="K1+7"),
    "persistent role=3 her2k K1=2BK K=4BK": dict(BULK, role=3, K1="2*BK", K="2*K1", her2k=1),
    "persistent role=1": dict(BULK, role=1, K="4*BK"),
    "persistent role=2 K=40": dict(BULK, role=2, K=40),
    "persistent role=3 rect": dict(BULK, role=3, rect=1, nt=17, nt_c=19, last_cols=5, K="2*BK"),
    "persistent role=4 adds": dict(BULK, role=4, K="2*BK"),
    "persistent nb=256 ld=129-unaligned": dict(BULK, nb=256, nt=12, ldc=257, ld=257, role=0, K="2*BK"),
    "persistent pr=2 pc=3 ri=1 ci=2 K1=24 K=48": dict(BULK, nt=49, pr=2, pc=3, ri=1, ci=2, role=0, K1=24, K="2*K1"),
    "persistent repeated with dirty counters": dict(BULK, role=0, K="8*BK", repeat=True),
    "persistent info!=0": dict(BULK, role=0, info=-5),
}

GRIDS = {}
for _pr, _pc in ((2, 2), (2, 3), (3, 2)):
    for _ri in range(_pr):
        for _ci in range(_pc):
            # 13 global tiles, ragged last one; tiles of 3 / 4 blocks so that the local domain has 16 block rows and
            # more: 8 x 8 patches, colstart, il_first
            GRIDS[f"grid pr={_pr} pc={_pc} ri={_ri} ci={_ci}"] = dict(
                nb=384 if _pr == 2 else 512, nt=13, last_rows=37, pr=_pr, pc=_pc, ri=_ri, ci=_ci, K=40, role=0,
                tile_layout=True, expect="plain")
            GRIDS[f"grid nb=128 pr={_pr} pc={_pc} ri={_ri} ci={_ci} K1=24"] = dict(
                nb=128, nt=13, last_rows=37, pr=_pr, pc=_pc, ri=_ri, ci=_ci, K1=24, K="K1+7", role=0, tile_layout=True)

UNIFORM = {
    "uniform nb=192 K=40": dict(SMALL, K=40),
    "uniform nb=128 role=1 K=512 preload": dict(nb=128, nt=3, role=1, K=512),
    "uniform nb=129 non-VEC K=40": dict(nb=129, last_rows=1, K=40),
    "uniform two-segment K1=24 K=31": dict(SMALL, K1=24, K="K1+7"),
    "uniform her2k K1=3BK K=6BK": dict(nb=256, nt=3, last_rows=37, K1="3*BK", K="2*K1", her2k=1, role=3),
    "uniform role=4 adds K=2BK": dict(SMALL, role=4, K="2*BK"),
    # 17 block rows: 6 patches, 384 work items (z: 768)
    "uniform persistent role=0 UTAIL K=4BK": dict(nb=128, nt=17, last_rows=37, max_blocks=16, role=0, K="4*BK",
                                                  expect="persistent"),
}


def params(cases):
    return [pytest.param(t, name, id=f"{name}, {t}") for name in cases for t in TYPES]


@gpu
@pytest.mark.parametrize("t,name", params(PLAIN))
def test_update_plain_exact(dlaf, t, name):
    run_case(dlaf, t, PLAIN[name])


@gpu
@pytest.mark.parametrize("t,name", params(GRIDS))
def test_update_process_grids_exact(dlaf, t, name):
    run_case(dlaf, t, GRIDS[name])


@gpu
@pytest.mark.parametrize("t,name", params(PERSISTENT))
def test_update_persistent_exact(dlaf, t, name):
    run_case(dlaf, t, PERSISTENT[name])


@gpu
@pytest.mark.parametrize("t", TYPES)
def test_update_exclusive_compute_units_exact(dlaf, t):
    """max_blocks = this GPU's workgroup slots and one whole round of exclusive compute units, on the smallest square
    tile count whose blocks -- a lower bound of the work items -- outnumber the slots."""
    slots = dlaf.update_bulk_slots(DT[t])
    assert slots > 0
    per_tile = (128 // BLK[t][0]) * (128 // BLK[t][1])
    nt = next(n for n in range(2, 200) if n * (n + 1) // 2 * per_tile > slots)
    run_case(dlaf, t, dict(nt=nt, last_rows=37, role=0, K="4*BK", max_blocks=-1, excl_rounds=1, expect="exclusive"))


@gpu
@pytest.mark.parametrize("t,name", params(UNIFORM))
def test_update_uniform_componentwise_bound(dlaf, t, name):
    run_case(dlaf, t, UNIFORM[name], kind="uniform")


def test_exact_operands_are_exact_at_the_largest_K():
    """No GPU: reference() itself asserts, tile by tile, that the sum in the working precision equals the sum in the
    wider type; here at K = 512 for all four types, with and without a second segment."""
    for t in TYPES:
        for spec in (dict(nb=64, nt=2, K=512), dict(nb=64, nt=2, K1=256, K=512, her2k=1)):
            reference(t, resolve(t, spec), "exact", np.random.default_rng(1), wide_exact=True)


SWITCH_CHILD = r"""
import sys, traceback
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import dla_future_amd as dl
import test_gpu_update_kernel as m
dl.initialize()
failed = 0
for name in %r:
    for t in m.TYPES:
        try:
            m.run_case(dl, t, m.PERSISTENT[name])
        except BaseException as e:
            failed += 1
            print("FAILED:", name + ",", t, "--", str(e)[:600], flush=True)
print("DONE", failed, flush=True)
"""
# K >= 8 BK: a start slab other than 0 and the wrap-around are possible under K-phase alignment
SWITCH_CASES = ["persistent max_blocks=8 role=0 UTAIL", "persistent max_blocks=16 role=0 UTAIL",
                "persistent role=3 her2k K1=2BK K=4BK", "persistent role=4 adds",
                "persistent pr=2 pc=3 ri=1 ci=2 K1=24 K=48", "persistent repeated with dirty counters"]


@gpu
@pytest.mark.parametrize("switch", ["DLAF_MI355X_KPHASE=1", "DLAF_MI355X_LOCKSTEP=1", "DLAF_MI355X_STEAL=0"])
def test_update_process_wide_switches_exact(switch):
    """The switches are read once per process: each runs in one child process of its own, on persistent cases with
    exact operands, and must give the same bits as the reference."""
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, "-c", SWITCH_CHILD % (ROOT, os.path.join(ROOT, "tests"), SWITCH_CASES)],
                       cwd=ROOT, env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "DONE 0" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
