"""World size 2 over gloo on one GPU (the pattern of tests/test_gpu_dist.py) with DPM-Solver++ 2M and Euler-ancestral: the
history ring and the counter-based noise keep every rank's latents bit-identical, and equal to the single-process loop."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,graphs", [("dpm", 1), ("euler_a", 1), ("lms", 0)])
def test_two_ranks_step_identically(name, graphs):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "sched_dist_gpu_worker.py"), name, str(graphs)],
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and f"SCHED_DIST_OK {name}" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
