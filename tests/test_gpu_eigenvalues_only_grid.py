"""The eigenvalues-only entries and the partial spectrum selected by value on a 2 x 3 process grid: six ranks on the one
GPU over gloo (tests/eigenvalues_only_dist_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_workers(nprow, npcol, order="R", timeout=600):
    from conftest import gpu_process_budget
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed import free_port
    n = nprow * npcol
    gpu_process_budget(n)
    port = str(free_port())
    procs = []
    for rank in range(n):
        env = dict(os.environ, OMP_NUM_THREADS="1", DLAF_MI355X_DEVICE="0", RANK=str(rank), WORLD_SIZE=str(n),
                   LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "eigenvalues_only_dist_worker.py"),
                                       str(nprow), str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    rc = [p.returncode for p in procs]
    assert all(r == 0 for r in rc) and "EIGENVALUES_ONLY_WORKER_RESULT OK" in outs[0][0], \
        (rc, "\n".join(o[0][-1500:] for o in outs), "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
def test_eigenvalues_only_and_by_value_on_a_six_rank_grid():
    launch_workers(2, 3)
