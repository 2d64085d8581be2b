"""The weighted Hermitian rank-k update and hermitian_function on process grids
(tests/weighted_rank_update_dist_worker.py): trans N on 1 x 2, 2 x 1, 2 x 2 and 2 x 3, d and z, both uplo, exact operands
over several SUMMA steps (the weight pointer advances per step), zero and non-zero source processes, host and resident
entries; hermitian_function with x^(-1/2) against the reference of test_gpu_hermitian_function.py.  Trans C on a grid is
refused before the GPU is touched."""
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
    assert n <= 6
    gpu_process_budget(n)
    port = str(free_port())
    procs = []
    outs = []
    try:
        for rank in range(n):
            env = dict(os.environ, OMP_NUM_THREADS="1", DLAF_MI355X_DEVICE="0", RANK=str(rank), WORLD_SIZE=str(n),
                       LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "weighted_rank_update_dist_worker.py"),
                                           str(nprow), str(npcol), order], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.PIPE, text=True))
        for p in procs:
            outs.append(p.communicate(timeout=timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    rc = [p.returncode for p in procs]
    assert all(r == 0 for r in rc) and "WEIGHTED_WORKER_RESULT OK" in outs[0][0], \
        (rc, "\n".join(o[0][-1500:] for o in outs), "\n".join(o[1][-1500:] for o in outs))


@pytest.mark.many_ranks
def test_weighted_rank_update_grid_2x3():
    launch_workers(2, 3)


# fresh_parent: the worker processes run about ten times slower once this pytest process has done GPU work of its own
# (conftest.py)
@pytest.mark.fresh_parent
@pytest.mark.parametrize("nprow,npcol", [(1, 2), (2, 1), (2, 2)])
def test_weighted_rank_update_grid(nprow, npcol):
    launch_workers(nprow, npcol)


def test_trans_c_on_a_grid_is_refused():
    """a 2 x 2 host grid on which no broadcast is ever made: the refusal comes before the GPU is touched"""
    code = ("import numpy as np, dla_future_amd as d\n"
            "g = d.Grid.host(4, 0, 2, 2, 'R', lambda axis, root, buf: None)\n"
            "a = np.ones((4, 6), order='F'); c = np.zeros((6, 6), order='F')\n"
            "d.hermitian_weighted_rank_k_update(g, 'L', 'C', 1.0, a, np.ones(4), 0.0, c, 2, n=6, k=4)\n"
            "print('survived')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert r.returncode != 0 and "survived" not in r.stdout, (r.stdout, r.stderr[-500:])
    assert "hermitian weighted rank-k update: trans 'C' on a 2 x 2 grid: only 'N' is built on more than one process" \
        in r.stderr, r.stderr[-500:]
