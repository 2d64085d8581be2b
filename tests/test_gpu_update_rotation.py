"""The fp64 update kernel after the fragment rotation of its K loop (csrc/device/mma_core.hpp, mma_slab_rotated) gives
the bits it gave before.

The rotation changes when a wave reads its MFMA fragments from LDS and in which order the 16 MFMAs of a k-step run; every
accumulator still receives the same products in ascending k from the same instruction.  So the property is bit identity
with the commit before the change.  tests/golden/update_rotation_bits.json holds, per case, the SHA-256 of the C buffer
that commit's kernel returned on an MI355X plus 16 sampled elements (our own kernel's outputs; written by
`python tests/test_gpu_update_rotation.py OUT.json` run against a build of that commit).  Each case is also checked
against numpy with the component-wise bound of tests/test_gpu_update_kernel.py, c (K + 2) u (|C0| + |A| |B|^H), so a
wrong golden cannot hide and the test keeps a meaning when a later compiler changes the bits.

Cases: fp64, nb = 128 (one 128 x 128 block per tile), ldc = nb, uniform operands in [-1, 1), lower-triangular domain
with its diagonal tiles (herk mask).  K = 16, 32, 48, 256 are one slab (no loop iteration), an even and an odd slab count,
and the two-slab ring wrapping many times.
  * role 0 persistent (the UTAIL form of the K loop), max_blocks = 8, asserted persistent through update_launch_stats.
    A launch goes persistent only with more work items than max_blocks, and 3 x 2 tiles hold 5: these cases run on
    5 x 2 tiles (9 work items on 8 workgroups, so one workgroup also reuses its ring for a second block).
  * role 0 two-segment K1 = 16, K = 48, persistent, same geometry.
  * role 0 plain on 3 x 2 tiles (one block per workgroup: the K loop that stops loading in its last iteration).
  * role 1 on 3 x 2 tiles: C preloaded into the accumulators, subtracting MFMAs (off-diagonal tiles).
  * role 4 (adds), K = 32, 3 x 2 tiles.
  * the race screen: 6 x 6 tiles, K = 256, persistent, 20 launches on restored C, one digest.  A read of a ring slot
    that is still in flight at the slab barrier, or issued ahead of it, shows as a launch whose bits differ.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "update_rotation_bits.json")
gpu = pytest.mark.gpu

NB = 128
LD_WIDER = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
RACE_LAUNCHES = 20

CASES = {}
for _k in (16, 32, 48, 256):
    CASES[f"role0 persistent K={_k}"] = dict(rows=5, cols=2, role=0, K=_k, max_blocks=8, persistent=True)
CASES["role0 persistent two-segment K1=16 K=48"] = dict(rows=5, cols=2, role=0, K=48, K1=16, max_blocks=8, persistent=True)
for _k in (16, 32, 48, 256):
    CASES[f"role0 plain K={_k}"] = dict(rows=3, cols=2, role=0, K=_k)
for _k in (16, 32, 48, 256):
    CASES[f"role1 preload K={_k}"] = dict(rows=3, cols=2, role=1, K=_k)
CASES["role4 adds K=32"] = dict(rows=3, cols=2, role=4, K=32)
RACE = "race screen 6x6 persistent K=256"
CASES[RACE] = dict(rows=6, cols=6, role=0, K=256, max_blocks=8, persistent=True)


def operands(name):
    """The flat host arrays of a case (c0, a, b, a2, b2) and the fields of the launch, seeded by the case's name."""
    s = CASES[name]
    rows, cols, K, K1 = s["rows"], s["cols"], s["K"], s.get("K1", 0)
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    rng = np.random.default_rng(seed)
    k1 = K1 if K1 > 0 else K
    kp = max(k1, K - k1)          # columns every panel tile holds
    tile_a = NB * kp
    c_tsr, c_tsc = NB * NB, NB * NB * rows
    c0 = rng.uniform(-1, 1, size=c_tsc * cols)
    a = rng.uniform(-1, 1, size=tile_a * rows)
    b = rng.uniform(-1, 1, size=tile_a * cols)
    a2 = rng.uniform(-1, 1, size=tile_a * rows) if K1 > 0 else None
    b2 = rng.uniform(-1, 1, size=tile_a * cols) if K1 > 0 else None
    fields = dict(il0=0, il1=rows, jl0=0, jl1=cols, nb=NB, K=K, K1=K1, pr=1, ri=0, pc=1, ci=0, nt=rows, last_rows=NB,
                  rect=0, nt_c=0, last_cols=0, her2k=0, b_period=1, b_jl0=-1, info=0, role=s["role"],
                  max_blocks=s.get("max_blocks", 0), excl_rounds=0, ltr=rows, ltc=cols, tile_layout=0, b_ts=tile_a,
                  b_ts2=tile_a * cols, c_tsr=c_tsr, c_tsc=c_tsc, ldc=NB, a_ts=tile_a, lda=NB, ldb=NB)
    return (c0, a, b, a2, b2), fields


def launch(dlaf, name, ops, fields):
    c0, a, b, a2, b2 = ops
    got = c0.copy()
    before = dlaf.update_launch_stats()[0]
    persistent, _, _ = dlaf.update_direct(got, a, b, a2=a2, b2=b2, **fields)
    after = dlaf.update_launch_stats()[0]
    want = 1 if CASES[name].get("persistent") else 0
    assert (persistent, after - before) == (want, want), (name, persistent, after - before)
    return got


def sample_indices(name, size):
    seed = int.from_bytes(hashlib.sha256(("samples " + name).encode()).digest()[:4], "little")
    return np.sort(np.random.default_rng(seed).choice(size, size=16, replace=False))


def record(name, got):
    idx = sample_indices(name, got.size)
    return dict(sha256=hashlib.sha256(got.tobytes()).hexdigest(),
                samples=[[int(i), float(got[i]).hex()] for i in idx])


def check_against_numpy(name, ops, fields, got):
    """Component-wise: |got - ref| <= (K + 2) u (|C0| + |A| |B|^T) on the elements the contract updates (the lower
    triangle of diagonal tiles, all of the tiles below), everything else bit for bit as it was."""
    c0, a, b, a2, b2 = ops
    rows, cols, K, K1 = fields["il1"], fields["jl1"], fields["K"], fields["K1"]
    k1 = K1 if K1 > 0 else K
    k2 = K - k1
    kp = max(k1, k2)
    hp = np.longdouble if LD_WIDER else np.float64
    kf = K + 2 if LD_WIDER else K + 3
    u = np.finfo(np.float64).eps / 2
    sign = 1 if fields["role"] == 4 else -1
    tile = lambda flat, i: flat[i * NB * kp:(i + 1) * NB * kp].reshape(kp, NB).T  # [row, k]
    cview = lambda flat, il, jl: flat[il * fields["c_tsr"] + jl * fields["c_tsc"]:][:NB * NB].reshape(NB, NB).T
    untouched = np.ones(c0.size, dtype=bool)
    worst = 0.0
    for il in range(rows):
        for jl in range(cols):
            if il < jl:
                continue
            diag = il == jl
            segs = [(tile(a, il)[:, :k1], (tile(a, il) if diag else tile(b, jl))[:, :k1])]
            if k2:
                segs.append((tile(a2, il)[:, :k2], (tile(a2, il) if diag else tile(b2, jl))[:, :k2]))
            cv = cview(c0, il, jl)
            ref = cv.astype(hp) + sign * sum(x.astype(hp) @ y.astype(hp).T for x, y in segs)
            bnd = kf * u * (np.abs(cv) + sum(np.abs(x) @ np.abs(y).T for x, y in segs))
            upd = np.tril(np.ones((NB, NB), dtype=bool)) if diag else np.ones((NB, NB), dtype=bool)
            cview(untouched, il, jl)[upd] = False
            err = np.abs(cview(got, il, jl).astype(hp) - ref).astype(np.float64)
            ratio = np.where(upd, err / bnd, 0.0)
            worst = max(worst, float(ratio.max()))
            if ratio.max() > 1.0:
                r, c = np.unravel_index(np.argmax(ratio), ratio.shape)
                pytest.fail(f"{name}: tile ({il},{jl}) element ({r},{c}): |got - ref| = {err[r, c]:.3e} is "
                            f"{ratio[r, c]:.2f} x the bound {bnd[r, c]:.3e}")
    changed = np.flatnonzero((got.view(np.uint64) != c0.view(np.uint64)) & untouched)
    assert changed.size == 0, f"{name}: {changed.size} elements outside the contract changed; first at {changed[0]}"
    print(f"{name}: max |got - ref| / bound = {worst:.3f}")


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def compare_with_golden(name, got, gold, label=""):
    rec = record(name, got)
    differing = [(i, v, w) for (i, v), (_, w) in zip(rec["samples"], gold["samples"]) if v != w]
    print(f"{name}{label}: sha256 {rec['sha256']} (golden {gold['sha256']}), {len(differing)} of 16 samples differ")
    assert [i for i, _ in rec["samples"]] == [i for i, _ in gold["samples"]], "the golden file samples other elements"
    assert not differing, f"{name}{label}: sampled elements differ from the parent's (index, got, parent): {differing[:4]}"
    assert rec["sha256"] == gold["sha256"], f"{name}{label}: the C buffer differs from the parent's bits"


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != RACE])
def test_update_rotation_bit_identical(dlaf, golden, name):
    ops, fields = operands(name)
    got = launch(dlaf, name, ops, fields)
    check_against_numpy(name, ops, fields, got)
    compare_with_golden(name, got, golden[name])


@gpu
def test_update_rotation_race_screen(dlaf, golden):
    """20 launches of one persistent case on restored C: every launch must give the one digest."""
    ops, fields = operands(RACE)
    first = launch(dlaf, RACE, ops, fields)
    check_against_numpy(RACE, ops, fields, first)
    compare_with_golden(RACE, first, golden[RACE], " launch 1")
    want = golden[RACE]["sha256"]
    for i in range(2, RACE_LAUNCHES + 1):
        got = launch(dlaf, RACE, ops, fields)
        digest = hashlib.sha256(got.tobytes()).hexdigest()
        if digest != want:
            bad = np.flatnonzero(got.view(np.uint64) != first.view(np.uint64))
            pytest.fail(f"launch {i} of {RACE_LAUNCHES}: {bad.size} elements differ from launch 1; first at {bad[0]}")


def test_golden_file_covers_the_cases():
    """No GPU: the golden file names exactly the cases of this module, 16 samples each at the indices drawn here."""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(CASES)
    for name, rec in gold.items():
        ops, _ = operands(name)
        assert len(rec["sha256"]) == 64
        assert [i for i, _ in rec["samples"]] == [int(i) for i in sample_indices(name, ops[0].size)]


if __name__ == "__main__":
    # write the golden file from the build on sys.path (run against a build of the commit before the rotation)
    sys.path.insert(0, os.environ.get("DLAF_PACKAGE_ROOT", ROOT))
    import dla_future_amd as dl
    dl.initialize()
    out = {}
    for case in CASES:
        case_ops, case_fields = operands(case)
        res = launch(dl, case, case_ops, case_fields)
        check_against_numpy(case, case_ops, case_fields, res)
        out[case] = record(case, res)
        if case == RACE:
            for _ in range(RACE_LAUNCHES - 1):
                again = launch(dl, case, case_ops, case_fields)
                assert hashlib.sha256(again.tobytes()).hexdigest() == out[case]["sha256"], "the build is not deterministic"
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", sys.argv[1], "from", dl.lib_path())
