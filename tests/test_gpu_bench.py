"""bench.py on the GPU: a plain run times exactly --steps loop iterations, carries the headline figures and none of the --full
extras, and --dump-outputs writes the denoised latents of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_is_lean_and_dumps_the_latents(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= res.keys()
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["dtype"] == "bf16"
    assert "roofline" not in res and "cpu_baseline" not in res and "parity" not in res
    assert res["config"]["whole_clips_after_timed_region"] is None and res["config"]["clocks"] is None
    lat = np.load(tmp_path / "latents.npy")
    assert lat.dtype == np.float32 and lat.shape == (1, 4, 12, 64, 64) and np.isfinite(lat).all()
