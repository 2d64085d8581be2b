"""The fp64 update kernel's direct-to-LDS K loop after its address arithmetic moved to per-slab scalar bases
(csrc/device/glds_addr.hpp, gemm_nt_block in csrc/device/mma_core.hpp): every load still reads the column it read before.

All cases go through dlaf.update_direct, one launch each, with the exact operands of tests/test_gpu_update_kernel.py
(multiples of 2^-6 in [-1, 1]: every product and partial sum is representable, so any summation order gives the same
bits) and are compared for equality with that module's numpy reference; every element outside the contract must come
back bit for bit.  A load that fetched another column, another segment or another operand's leading dimension changes
whole accumulator rows, not last bits.  The arithmetic itself is swept on the CPU (tests/test_glds_addr.py).

fp64, full tiles (the direct-to-LDS path), nb = 128 (one block per tile) and 256 (four), 3 x 2 tiles (one block per
workgroup) and 5 x 2 tiles (persistent at max_blocks = 8, asserted through update_launch_stats):
  * K = 16, 32, 48, 256: one slab (no loop iteration loads anything new), two, three, many;
  * the rectangular form with lda != ldb;
  * two segments and her2k with K1 = BK and 3 BK, the second panel in the same device allocation as the first and in
    front of it, so that its address is the lower one;
  * roles 0 (plain and persistent), 1 (C preloaded into the accumulators) and 4 (adds);
  * DLAF_MI355X_KPHASE=1 (the sum starts at a slab other than 0 and wraps) in one child process, 3 and 16 slabs;
  * 20 launches of one persistent case: one digest.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_update_kernel as uk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
BK = uk.BLK["d"][2]
KS = (BK, 2 * BK, 3 * BK, 16 * BK)


def tiles3x2(nb, **kw):
    return dict(dict(nb=nb, nt=3, jl1=2, expect="plain"), **kw)


def tiles5x2(nb, **kw):
    return dict(dict(nb=nb, nt=5, jl1=2, max_blocks=8, expect="persistent"), **kw)


CASES = {}
for _nb in (128, 256):
    for _k in KS:
        CASES[f"nb={_nb} K={_k} role=0 persistent"] = tiles5x2(_nb, K=_k, role=0)
        CASES[f"nb={_nb} K={_k} role=0 plain"] = tiles3x2(_nb, K=_k, role=0)
        CASES[f"nb={_nb} K={_k} role=1 preload"] = tiles3x2(_nb, K=_k, role=1)
    for _k in (BK, 3 * BK):
        CASES[f"nb={_nb} K={_k} role=4 adds"] = tiles3x2(_nb, K=_k, role=4)
    # rectangular form, lda != ldb (ldb_pad widens the column panel's leading dimension; 16-byte alignment kept)
    CASES[f"nb={_nb} rect 3x2 role=3 K=48 lda!=ldb"] = tiles3x2(_nb, rect=1, nt_c=2, last_cols=_nb, role=3, K=3 * BK, ldb_pad=8)
    CASES[f"nb={_nb} rect 5x2 role=0 persistent K=256 lda!=ldb"] = tiles5x2(_nb, rect=1, nt_c=2, last_cols=_nb, role=0,
                                                                           K=16 * BK, ldb_pad=24)
    CASES[f"nb={_nb} 5x2 role=0 persistent K=48 lda!=ldb"] = tiles5x2(_nb, role=0, K=3 * BK, ldb_pad=8)
    # two segments / her2k, the second panel below the first
    for _k1 in (BK, 3 * BK):
        _two = dict(K1=_k1, K=4 * BK, second_below=1)
        CASES[f"nb={_nb} two-segment K1={_k1} K=64 role=0 plain"] = tiles3x2(_nb, role=0, **_two)
        CASES[f"nb={_nb} two-segment K1={_k1} K=64 role=0 persistent"] = tiles5x2(_nb, role=0, **_two)
        CASES[f"nb={_nb} two-segment K1={_k1} K=64 role=1 preload"] = tiles3x2(_nb, role=1, **_two)
        CASES[f"nb={_nb} her2k K1={_k1} K=64 role=3 plain"] = tiles3x2(_nb, role=3, her2k=1, **_two)
        CASES[f"nb={_nb} her2k K1={_k1} K=64 role=3 persistent"] = tiles5x2(_nb, role=3, her2k=1, **_two)
KPHASE_CASES = [f"nb={_nb} K={_k} role=0 persistent" for _nb in (128, 256) for _k in (3 * BK, 16 * BK)] + \
               ["nb=128 two-segment K1=16 K=64 role=0 persistent", "nb=256 her2k K1=48 K=64 role=3 persistent",
                "nb=256 rect 5x2 role=0 persistent K=256 lda!=ldb"]
RACE = "nb=256 K=256 role=0 persistent"
RACE_LAUNCHES = 20


def widen(flat, ld, kp, pad, sentinel):
    """A panel of [k][ld] tiles laid out again with leading dimension ld + pad, the padding holding the sentinel."""
    ntiles = flat.size // (ld * kp)
    out = np.full(ntiles * (ld + pad) * kp, sentinel, dtype=flat.dtype)
    out.reshape(ntiles, kp, ld + pad)[:, :, :ld] = flat.reshape(ntiles, kp, ld)
    return out


def build(name):
    """Operands, launch fields and expectation of a case: everything but the launch, so that repeated launches share it."""
    spec = dict(CASES[name])
    pad, below = spec.pop("ldb_pad", 0), spec.pop("second_below", 0)
    s = uk.resolve("d", spec)
    seed = int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")
    (c0, a, b, a2, b2), want, mask, _, geo = uk.reference("d", s, "exact", np.random.default_rng(seed))
    if pad:
        kp = geo["a_ts"] // geo["lda"]
        sent = np.float64(uk.SENTINEL[False])
        b = widen(b, geo["ldb"], kp, pad, sent)
        b2 = widen(b2, geo["ldb"], kp, pad, sent) if b2 is not None else None
        ratio = (geo["ldb"] + pad, geo["ldb"])
        geo = dict(geo, ldb=geo["ldb"] + pad, b_ts=geo["b_ts"] * ratio[0] // ratio[1], b_ts2=geo["b_ts2"] * ratio[0] // ratio[1])
    fields = {k: s[k] for k in ("il0", "il1", "jl0", "jl1", "nb", "K", "pr", "ri", "pc", "ci", "nt", "last_rows", "rect",
                                "nt_c", "last_cols", "K1", "her2k", "b_period", "b_jl0", "info", "role", "max_blocks",
                                "excl_rounds", "ltr", "ltc")}
    fields.update(tile_layout=0, second_below=below, **{k: geo[k] for k in ("b_ts", "b_ts2", "c_tsr", "c_tsc", "ldc",
                                                                            "a_ts", "lda", "ldb")})
    return dict(name=name, ops=(c0, a, b, a2, b2), want=want, mask=mask, fields=fields,
                persistent=1 if s["expect"] == "persistent" else 0)


def launch(dlaf, case):
    """One launch on a fresh copy of C; asserts the form the launch took, returns the C buffer."""
    c0, a, b, a2, b2 = case["ops"]
    got = c0.copy()
    before = dlaf.update_launch_stats()[0]
    persistent, _, _ = dlaf.update_direct(got, a, b, a2=a2, b2=b2, **case["fields"])
    after = dlaf.update_launch_stats()[0]
    assert (persistent, after - before) == (case["persistent"],) * 2, (case["name"], persistent, after - before)
    return got


def check(case, got):
    c0, want, mask = case["ops"][0], case["want"], case["mask"]
    assert mask.any()
    np.testing.assert_array_equal(got.view(np.uint64)[~mask], c0.view(np.uint64)[~mask],
                                  err_msg=f"{case['name']}: elements outside the contract changed")
    np.testing.assert_array_equal(got[mask], want[mask], err_msg=f"{case['name']}: updated elements differ")


@pytest.fixture(scope="module")
def dlaf():
    import dla_future_amd as d
    d.initialize()
    return d


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_update_slab_bases_exact(dlaf, name):
    case = build(name)
    check(case, launch(dlaf, case))


@gpu
def test_update_slab_bases_repeated_launches_one_digest(dlaf):
    """20 launches of one persistent case on restored C: the reference's bits every time."""
    case = build(RACE)
    first = launch(dlaf, case)
    check(case, first)
    want = hashlib.sha256(first.tobytes()).hexdigest()
    for i in range(2, RACE_LAUNCHES + 1):
        got = launch(dlaf, case)
        if hashlib.sha256(got.tobytes()).hexdigest() != want:
            bad = np.flatnonzero(got.view(np.uint64) != first.view(np.uint64))
            pytest.fail(f"launch {i} of {RACE_LAUNCHES}: {bad.size} elements differ from launch 1; first at {bad[0]}")


KPHASE_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import dla_future_amd as dl
import test_gpu_update_slab_bases as m
dl.initialize()
failed = 0
for name in m.KPHASE_CASES:
    try:
        case = m.build(name)
        m.check(case, m.launch(dl, case))
    except BaseException as e:
        failed += 1
        print("FAILED:", name, "--", str(e)[:600], flush=True)
print("DONE", failed, flush=True)
"""


@gpu
def test_update_slab_bases_kphase_exact():
    """K-phase alignment is read once per process: one child process runs persistent cases of 3 and 16 slabs (and 4 in
    two segments) with it on; the start slab and the wrap-around depend on the clock, the bits must not."""
    r = subprocess.run([sys.executable, "-c", KPHASE_CHILD % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT,
                       env=dict(os.environ, DLAF_MI355X_KPHASE="1"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "DONE 0" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_cases_cover_what_the_module_says():
    """No GPU: the case table holds every K, both tile sizes, both geometries and every role named above, and the
    reference builds (and is exact) for every case."""
    for nb in (128, 256):
        for k in KS:
            for form in ("role=0 persistent", "role=0 plain", "role=1 preload"):
                assert f"nb={nb} K={k} {form}" in CASES
    assert all(n in CASES for n in KPHASE_CASES) and RACE in CASES
    for name in CASES:
        case = build(name)
        assert case["persistent"] == (1 if "persistent" in name else 0)
        assert case["fields"]["ldb"] != case["fields"]["lda"] or "lda!=ldb" not in name
