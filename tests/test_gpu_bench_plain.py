"""`python bench.py --gpus 1 --steps K --warmup W` as the driver starts it: the real engine on one card, and a line that carries the headline and
the rooflines stamped inside the timed steps, nothing that takes a run of its own (that is --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                 "data", "rccl_ranks", "backend", "config", "roofline", "roofline_north_star", "roofline_attention"}


def test_plain_bench_run_prints_the_headline_alone(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                             "V3D_BENCH_DRY", "V3D_BENCH_REHEARSAL", "V3D_BENCH_FORCE_DIST")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert set(d) == HEADLINE_KEYS, sorted(set(d) ^ HEADLINE_KEYS)
    assert d["metric"] == "scenes/sec ScanQA @32 frames" and d["unit"] == "scenes/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["data"] == "synthetic"
    assert d["value"] > 0 and abs(d["value"] - 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "roofline_north_star", "roofline_attention"):
        assert d[k]["us_per_launch"] > 0
    ids = np.load(tmp_path / "answer_token_ids.npy")
    assert ids.dtype == np.float64 and ids.shape == (2, 17)
