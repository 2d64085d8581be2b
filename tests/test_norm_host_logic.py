"""CPU tests of the host side of the matrix norms (no GPU): the entries are exported and typed; a bad norm / uplo / diag
character, a descriptor the routines do not take and a source process outside the grid come back as their negative code,
and an empty matrix as 0, all without HIP being initialised (the child processes see no device, so any HIP call would
terminate them); and the work split and the partial-buffer layout of the kernels (csrc/device/norm_split.hpp) pass the
stand-alone sweep tests/norm_split/sweep.cpp -- every referenced element covered exactly once, every partial slot with
exactly one writer, pass 2 reading written slots only -- plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "norm_split", "sweep.cpp")
INC = os.path.join(ROOT, "dla_future_amd", "csrc", "device")

ENTRIES = [f"dlaf_mi355x_{name}_norm_{t}" for name in ("general", "hermitian", "triangular") for t in "sdcz"] + \
          [f"dlaf_mi355x_p{t}lange" for t in "sdcz"] + [f"dlaf_mi355x_p{t}lantr" for t in "sdcz"] + \
          ["dlaf_mi355x_pslansy", "dlaf_mi355x_pdlansy", "dlaf_mi355x_pclanhe", "dlaf_mi355x_pzlanhe",
           "dlaf_mi355x_matrix_norm", "dlaf_mi355x_general_matrix_norm", "dlaf_mi355x_norm_profile",
           "dlaf_mi355x_gmatrix_device_tiles"]


def test_norm_entries_exported():
    import dla_future_amd as d
    from dla_future_amd.capi import SIGNATURES
    L = C.CDLL(d.lib_path())
    for name in ENTRIES:
        assert hasattr(L, name) and name in SIGNATURES, name
    for name in ("matrix_norm", "matrix_norm_device", "pxlange", "pxlanhe", "pxlantr", "norm_profile"):
        assert callable(getattr(d, name)) and name in d.__all__, name


def _run(code):
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))


PRELUDE = ("import numpy as np, ctypes as C, dla_future_amd as d\n"
           "from dla_future_amd.capi import lib, DLAFDescriptor\n"
           "g = d.Grid.single(); a = np.eye(6, order='F'); v = C.c_double(-7.0)\n"
           "def desc(m=6, n=6, mb=2, nb=2, isrc=0, jsrc=0, i=0, j=0, ld=6):\n"
           "    return DLAFDescriptor(m, n, mb, nb, isrc, jsrc, i, j, ld)\n"
           "G = lambda norm, da: lib().dlaf_mi355x_general_norm_d(g.context, norm, a.ctypes.data, da, C.byref(v))\n"
           "H = lambda norm, uplo, da: lib().dlaf_mi355x_hermitian_norm_d(g.context, norm, uplo, a.ctypes.data, da, C.byref(v))\n"
           "T = lambda norm, uplo, diag, da: lib().dlaf_mi355x_triangular_norm_d(g.context, norm, uplo, diag, a.ctypes.data, da,"
           " C.byref(v))\n")


def test_bad_arguments_return_their_codes_without_hip():
    r = _run(PRELUDE +
             "out = [G(b'X', desc()), H(b'Q', b'L', desc()), T(b'2', b'L', b'N', desc()),\n"          # -1 x 3
             "       H(b'M', b'X', desc()), T(b'M', b'G', b'N', desc()),\n"                          # -2 x 2
             "       T(b'M', b'L', b'X', desc()),\n"                                                 # -3
             "       G(b'M', desc(mb=3)), G(b'M', desc(nb=0, mb=0)), G(b'M', desc(i=1)), G(b'M', desc(m=-1)),\n"  # -4 x 4
             "       H(b'M', b'L', desc(m=6, n=4)), T(b'F', b'U', b'U', desc(m=4, n=6)),\n"          # -4 x 2
             "       G(b'M', desc(isrc=1)), H(b'M', b'L', desc(jsrc=2)),\n"                          # -5 x 2
             "       lib().dlaf_mi355x_general_norm_d(g.context, b'M', a.ctypes.data, desc(), None),\n"  # -6
             "       lib().dlaf_mi355x_general_norm_d(12345, b'M', a.ctypes.data, desc(), C.byref(v)),\n"  # -6
             "       lib().dlaf_mi355x_matrix_norm(None, b'M', b'H', b'N', C.byref(v)),\n"
             "       lib().dlaf_mi355x_general_matrix_norm(None, b'M', C.byref(v))]\n"
             "print('codes', out, v.value)")
    assert r.returncode == 0, (r.stdout, r.stderr[-800:])
    assert "codes [-1, -1, -1, -2, -2, -3, -4, -4, -4, -4, -4, -4, -5, -5, -6, -6, -1, -6] -7.0" in r.stdout, r.stdout
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


def test_empty_matrices_have_norm_zero_without_hip():
    r = _run(PRELUDE +
             "out = []\n"
             "for norm in (b'M', b'1', b'o', b'I', b'F', b'e'):\n"
             "    for da in (desc(m=0, n=6), desc(m=6, n=0), desc(m=0, n=0)):\n"
             "        v.value = -7.0; out.append((G(norm, da), v.value))\n"
             "    v.value = -7.0; out.append((H(norm, b'U', desc(m=0, n=0)), v.value))\n"
             "    v.value = -7.0; out.append((T(norm, b'L', b'U', desc(m=0, n=0)), v.value))\n"
             "assert all(o == (0, 0.0) for o in out), out\n"
             "assert d.matrix_norm(g, 'F', np.zeros((0, 5), order='F'), 2, m=0, n=5) == 0.0\n"
             "dd = [1, g.context, 0, 0, 2, 2, 0, 0, 1]\n"
             "assert d.pxlange('M', 0, 0, a, 1, 1, dd) == 0.0 and d.pxlanhe('1', 'L', 0, a, 1, 1, dd) == 0.0\n"
             "assert d.pxlantr('I', 'U', 'N', 0, a, 1, 1, dd) == 0.0\n"
             "print('all zero')")
    assert r.returncode == 0 and "all zero" in r.stdout, (r.stdout, r.stderr[-800:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


@pytest.mark.parametrize("call,needle", [
    ("d.pxlange('M', 4, 4, a, 2, 1, [1, g.context, 4, 4, 2, 2, 0, 0, 6])", "ia, ja must be 1"),
    ("d.pxlantr('Z', 'L', 'N', 4, a, 1, 1, [1, g.context, 4, 4, 2, 2, 0, 0, 6])", "bad argument (code -1"),
    ("d.pxlanhe('M', 'L', 4, a, 1, 1, [2, g.context, 4, 4, 2, 2, 0, 0, 6])", "(dtype) must be 1"),
])
def test_scalapack_entries_terminate_on_bad_arguments(call, needle):
    r = _run(PRELUDE + call + "\nprint('survived')")
    assert r.returncode != 0 and "survived" not in r.stdout and needle in r.stderr, (r.stdout, r.stderr[-500:])
    assert "HIP error" not in r.stderr and "no HIP device" not in r.stderr, r.stderr[-500:]


def test_norm_split_sweep_plain_and_sanitized(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    builds = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
    procs = {}
    for name, flags in builds.items():
        exe = str(tmp_path / f"sweep_{name}")
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True,
                       capture_output=True, text=True, timeout=300)
        procs[name] = subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, f"{name}: exit {p.returncode}\n{out}\n{err[-4000:]}"
        words = out.split()
        assert words[0] == "geometries" and int(words[1]) > 20000 and words[-2:] == ["failures", "0"], out
