"""The matrix norms on 2 x 3 and 3 x 2 process grids: six ranks on the one GPU over gloo (tests/norm_dist_worker.py).
Every norm of every structure for d and c at n = 400, nb = 128 with source rank (1, 2) / (2, 1), at n = 100, nb = 64
(some ranks own no tile and pass an empty local part) and for a general 400 x 130 matrix: exact operands against the
one-process reference, the max norm with the bits of a one-process run, identical bits on every rank, and a NaN owned by
the last rank reaching every rank."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_norm_workers(nprow, npcol, order="R", timeout=600):
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
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "norm_dist_worker.py"), str(nprow),
                                       str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
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
    assert all(r == 0 for r in rc) and "NORM_WORKER_RESULT OK" in outs[0][0], \
        (rc, "\n".join(o[0][-1500:] for o in outs), "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
@pytest.mark.parametrize("nprow,npcol", [(2, 3), (3, 2)])
def test_norms_on_a_six_rank_grid(nprow, npcol):
    launch_norm_workers(nprow, npcol)
