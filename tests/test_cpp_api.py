"""The C++ facade include/dlaf_mi355x/dlaf.hpp (the reference's C++ names over the C ABI): a C++17 program
patterned on test/unit/factorization/test_cholesky.cpp and test/unit/solver/test_triangular.cpp is compiled
with g++ here (CPU: the header is self-contained and links) and run on the GPU box."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "dla_future_amd", "lib")
HEADERS = [os.path.join(ROOT, "include", "dlaf_mi355x", h) for h in ("dlaf.hpp", "dlaf_mi355x.h")]
MINIAPPS = ["miniapp_cholesky", "miniapp_triangular_solver", "miniapp_triangular_multiplication",
            "miniapp_hermitian_multiplication", "miniapp_gen_to_std", "miniapp_inverse_from_cholesky_factor",
            "miniapp_reduction_to_band", "miniapp_eigensolver"]


def _stale(exe, sources):
    return not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in sources)


def build_cpp_test(name):
    """tests/cpp_api/<name>.cpp -> tests/cpp_api/<name>, rebuilt when the source or a facade header is newer."""
    src = os.path.join(ROOT, "tests", "cpp_api", name + ".cpp")
    exe = os.path.join(ROOT, "tests", "cpp_api", name)
    if _stale(exe, [src] + HEADERS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", LIB,
                        "-ldlaf_mi355x", f"-Wl,-rpath,{LIB}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_cpp_facade_compiles_and_links():
    assert os.path.exists(build_cpp_test("test_cholesky_cpp"))


def test_every_facade_template_instantiates_and_links_for_every_type():
    """instantiate_all.cpp instantiates every public template of the facade for s, d, c and z: a signature that moved
    fails the compilation, a missing or misspelt C entry of any type fails the link."""
    assert os.path.exists(build_cpp_test("instantiate_all"))


@pytest.mark.gpu
def test_reference_style_cpp_tests_on_the_facade():
    r = subprocess.run([build_cpp_test("test_cholesky_cpp")], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0 and "CPP_API_TEST OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def build_miniapp(mpi=False, name="miniapp_cholesky"):
    """miniapp/<name>.cpp -> miniapp/<name>[_mpi], rebuilt when the source, the shared miniapp header or a facade header
    is newer."""
    src = os.path.join(ROOT, "miniapp", name + ".cpp")
    exe = os.path.join(ROOT, "miniapp", name + ("_mpi" if mpi else ""))
    if not _stale(exe, [src, os.path.join(ROOT, "miniapp", "miniapp_common.hpp")] + HEADERS):
        return exe
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-L", LIB]
    if mpi:
        import test_c_api
        test_c_api.build("test_grid_mpi")   # makes sure the MPI shim and its private link directory exist
        inc = os.path.join(os.path.dirname(os.path.dirname(test_c_api.MPICC)), "include")
        cmd += ["-DDLAF_MI355X_WITH_MPI", "-I", inc, "-L", os.path.join(LIB, "mpi"), "-ldlaf_mi355x_mpi", "-lmpi",
                f"-Wl,-rpath-link,{LIB}/mpi", f"-Wl,-rpath,{LIB}/mpi"]
    cmd += ["-ldlaf_mi355x", f"-Wl,-rpath,{LIB}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_miniapp_compiles():
    for name in MINIAPPS:
        assert os.path.exists(build_miniapp(name=name))


# Only the five miniapps that mirror an upstream program print a usage line after an unknown option.
MINIAPP_USAGE = {
    "miniapp_cholesky": "usage: miniapp_cholesky --matrix-size N --block-size NB [--grid-rows R --grid-cols C]",
    "miniapp_gen_to_std": "usage: miniapp_gen_to_std --matrix-size N --block-size NB [--grid-rows R --grid-cols C]",
    "miniapp_inverse_from_cholesky_factor":
        "usage: miniapp_inverse_from_cholesky_factor --matrix-size N --block-size NB [--grid-rows R --grid-cols C]",
    "miniapp_reduction_to_band": "usage: miniapp_reduction_to_band --matrix-size N --block-size NB [--band-size B]",
    "miniapp_eigensolver": "usage: miniapp_eigensolver --matrix-size N --block-size NB [--band-size B]",
}


@pytest.mark.parametrize("name", MINIAPPS)
def test_miniapp_argument_errors(name):
    """The exits of the option parser and of the process-count check: status 2, nothing on stdout, one message on stderr.
    They all happen before dlaf::initialize(), so no GPU is touched."""
    exe = build_miniapp(name=name)

    def stderr_of(*args):
        r = subprocess.run([exe, *args], cwd=ROOT, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stdout == "", (args, r.returncode, r.stdout, r.stderr)
        return r.stderr

    unknown = stderr_of("--bogus").splitlines()
    assert unknown[0] == "unknown option --bogus", unknown
    if name in MINIAPP_USAGE:
        assert len(unknown) == 2 and unknown[1].startswith(MINIAPP_USAGE[name]) and unknown[1].endswith("[--csv]"), unknown
    else:
        assert len(unknown) == 1, unknown
    assert stderr_of("--nruns") == "missing value for --nruns\n"
    assert stderr_of("--nruns", "2", "--type") == "missing value for --type\n"
    assert stderr_of("--type", "q") == "invalid option value\n"
    assert stderr_of("--grid-rows", "2") == "grid 2 x 1 needs 2 processes, got 1\n"


def check_miniapp_output(out, nruns, nchecks):
    import re
    runs = re.findall(r"^\[(\d+)\] ([0-9.e+-]+)s ([0-9.e+-]+)GFlop/s (\w+) \((\d+), (\d+)\) \((\d+), (\d+)\) \((\d+), (\d+)\) 1 GPU$",
                      out, flags=re.M)
    assert len(runs) == nruns, out
    assert all(float(r[2]) > 0 for r in runs)
    assert out.count("CSVData-2, run, ") == nruns
    checks = re.findall(r"^(ERROR: |Warning: )?Max Diff / Max A: ([0-9.e+-]+)$", out, flags=re.M)
    assert len(checks) == nchecks and all(c[0] == "" for c in checks), out


@pytest.mark.gpu
def test_miniapp_cholesky_reference_cli_and_output():
    exe = build_miniapp()
    for t, uplo in (("d", "L"), ("z", "U")):
        r = subprocess.run([exe, "--matrix-size", "2048", "--block-size=256", "--nruns", "2", "--nwarmups", "1", "--type", t,
                            "--uplo", uplo, "--check-result", "all", "--csv"], cwd=ROOT, capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        check_miniapp_output(r.stdout, 2, 3)   # "all" also checks the warm-up run, as upstream does


@pytest.mark.gpu
def test_miniapp_cholesky_mpi_grid():
    import test_c_api
    exe = build_miniapp(mpi=True)
    env = dict(os.environ, DLAF_MI355X_MPI_TRANSPORT="host", DLAF_MI355X_DEVICE="0", OMP_NUM_THREADS="1")
    env.pop("LOCAL_RANK", None)
    r = subprocess.run([test_c_api.MPIEXEC, "-n", "4", exe, "--matrix-size", "1500", "--block-size", "128", "--grid-rows", "2",
                        "--grid-cols", "2", "--nruns", "2", "--check-result", "last", "--csv"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("GFlop/s d") == 2 and "(2, 2)" in r.stdout and "ERROR" not in r.stdout and \
        r.stdout.count("Max Diff / Max A") == 1, r.stdout


@pytest.mark.gpu
def test_miniapp_triangular_solver():
    import re
    exe = build_miniapp(name="miniapp_triangular_solver")
    r = subprocess.run([exe, "--m", "1500", "--n", "700", "--mb", "128", "--nb", "128", "--side", "L", "--uplo", "L", "--op", "N",
                        "--nruns", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s dLLNN \(1500, 700\) \(128, 128\) \(1, 1\) 1 GPU", r.stdout,
                          flags=re.M)) == 2, r.stdout
    resid = float(re.search(r"corner: ([0-9.e+-]+)", r.stdout).group(1))
    assert resid < 1e-11, r.stdout


@pytest.mark.gpu
def test_miniapp_gen_to_std():
    """miniapp_gen_to_std.cpp: the reference's options and result lines; both operands resident on the device."""
    import re
    exe = build_miniapp(name="miniapp_gen_to_std")
    for tp, uplo in (("d", "L"), ("z", "U")):
        r = subprocess.run([exe, "--matrix-size", "1500", "--block-size", "128", "--type", tp, "--uplo", uplo, "--nruns", "2",
                            "--csv"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s %s%s \(1500, 1500\) \(128, 128\) \(1, 1\) 1 GPU" % (tp, uplo),
                              r.stdout, flags=re.M)) == 2, r.stdout
        assert r.stdout.count("CSVData-2, run, ") == 2, r.stdout


@pytest.mark.gpu
def test_miniapp_reduction_to_band():
    """miniapp_reduction_to_band.cpp: the reference's options (incl. --band-size) and result lines; the matrix resident
    on the device in the timed window."""
    import re
    exe = build_miniapp(name="miniapp_reduction_to_band")
    for tp, band in (("d", "64"), ("z", "128")):
        r = subprocess.run([exe, "--matrix-size", "1500", "--block-size", "128", "--band-size", band, "--type", tp, "--nruns", "2",
                            "--csv"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s [0-9.e+-]+GFlop/s %s \(1500, 1500\) \(128, 128\) %s \(1, 1\) 1 GPU" % (tp, band),
                              r.stdout, flags=re.M)) == 2, r.stdout
        assert r.stdout.count("CSVData-2, run, ") == 2 and "band_size, " + band in r.stdout, r.stdout


@pytest.mark.gpu
def test_miniapp_eigensolver():
    """miniapp_eigensolver.cpp: the reference's options and result lines, its checker (--check-result) on one process."""
    import re
    exe = build_miniapp(name="miniapp_eigensolver")
    for tp in ("d", "z"):
        r = subprocess.run([exe, "--matrix-size", "700", "--block-size", "128", "--type", tp, "--nruns", "2", "--check-result", "last",
                            "--csv"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, DLAF_MI355X_DEVICE="0"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert len(re.findall(r"^\[\d+\] [0-9.e+-]+s %s \(700, 700\) \(128, 128\) \(1, 1\) 1 GPU" % tp, r.stdout, flags=re.M)) == 2, r.stdout
        assert r.stdout.count("Check: OK") == 1 and "Check: ERROR" not in r.stdout, r.stdout
        assert r.stdout.count("CSVData-2, run, ") == 2, r.stdout
