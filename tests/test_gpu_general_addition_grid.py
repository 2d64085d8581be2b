"""general_addition, hermitian_complete and the resident conversions on process grids (tests/addition_dist_worker.py):
1 x 2, 2 x 1, 2 x 2 and 2 x 3, d and z, exact operands at nb = 48, m = 357, n = 165 with non-zero source processes: op N
(local, no broadcast), op T and C (the transposed-panel walk) with uplo A and L, hermitian_complete for both uplo and
both kinds, both conversions from a U DeviceMatrix, host and resident entries; every rank compares its own local part
with equality and everything else bit for bit, and the communication logs of a communicator's members agree."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_addition_workers(nprow, npcol, order="R", timeout=600):
    from conftest import gpu_process_budget
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_distributed import free_port
    n = nprow * npcol
    assert n <= 6
    gpu_process_budget(n)
    port = str(free_port())
    procs = []
    outs = []
    try:
        for rank in range(n):
            env = dict(os.environ, OMP_NUM_THREADS="1", DLAF_MI355X_DEVICE="0", RANK=str(rank), WORLD_SIZE=str(n),
                       LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "addition_dist_worker.py"), str(nprow),
                                           str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True))
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    rc = [p.returncode for p in procs]
    assert all(r == 0 for r in rc) and "ADDITION_WORKER_RESULT OK" in outs[0][0], \
        (rc, "\n".join(o[0][-1500:] for o in outs), "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
def test_general_addition_grid_2x3():
    launch_addition_workers(2, 3)


# fresh_parent: the worker processes run about ten times slower once this pytest process has done GPU work of its own
# (conftest.py)
@pytest.mark.fresh_parent
@pytest.mark.parametrize("nprow,npcol", [(1, 2), (2, 1), (2, 2)])
def test_general_addition_grid(nprow, npcol):
    launch_addition_workers(nprow, npcol)
