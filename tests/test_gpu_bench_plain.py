"""A plain `bench.py` run (no --full) at a small shape: the headline fields only, exactly --steps timed steps, and
--dump-outputs writing the last timed eval step's result as float32 / float64 arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--queries", "40", "--rotate", "3", "--dump-outputs", str(dump)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "videos/sec (eval fwd)" and d["unit"] == "videos/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]
    assert d["eval_graphs"]["captures_in_timed_region"] == 0
    # what moved behind --full is not in a plain line
    for k in ("train_step_ms", "roofline", "kernels_us", "cpu_baseline", "shader_clock_mhz", "eval_strict_fp32"):
        assert k not in d, k
    files = sorted(os.listdir(dump))
    assert "eval.0.pred_boxes.npy" in files and "eval.0.pred_logits.npy" in files, files
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 * 2 ** 20 + 256 * len(files)
    for f in files:
        arr = np.load(dump / f)
        assert arr.dtype in (np.float32, np.float64), (f, arr.dtype)
        assert np.isfinite(arr).all(), f
    boxes = np.load(dump / "eval.0.pred_boxes.npy")
    assert boxes.shape[-1] == 2 and boxes.size == 4 * 40 * 2 and np.isfinite(boxes).all()
