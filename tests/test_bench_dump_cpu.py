"""bench.py --dump-outputs on the host side: what a step's result becomes on disk (names, dtypes, the 64 MB bound and its
seeded sample), and the argument checks that run before any device call.  The GPU run of the same path is
tests/test_gpu_bench_plain.py."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_arrays_names_and_dtypes():
    out = ({"pred_boxes": torch.rand(2, 3, 2), "seq": torch.tensor([[1, 7], [0, 3]]), "alive": torch.tensor([True, False]),
            "half": torch.rand(4, dtype=torch.bfloat16), "aux_outputs": [{"pred_logits": torch.rand(2, 1, dtype=torch.float64)}],
            "cl_match_mats": 0}, {"loss_ce": torch.tensor(0.5), "loss_self_iou": torch.tensor(float("nan")),
                                  "loss_self_iou_0": torch.tensor(float("nan"))})
    got = bench.host_arrays(out, "eval", {})
    assert sorted(got) == ["eval.0.alive", "eval.0.aux_outputs.0.pred_logits", "eval.0.half", "eval.0.pred_boxes",
                           "eval.0.seq", "eval.1.loss_ce"]
    assert got["eval.0.pred_boxes"].dtype == np.float32 and got["eval.0.half"].dtype == np.float32
    assert got["eval.0.aux_outputs.0.pred_logits"].dtype == np.float64
    assert got["eval.0.seq"].dtype == np.float64 and got["eval.0.seq"].tolist() == [[1, 7], [0, 3]]
    assert got["eval.0.alive"].tolist() == [1.0, 0.0] and got["eval.1.loss_ce"].shape == ()


def test_write_outputs_whole_and_sampled(tmp_path):
    rs = np.random.RandomState(3)
    arrays = {"eval.0.small": rs.rand(10).astype(np.float32), "eval.0.big": rs.rand(4000).astype(np.float32)}
    bench.write_outputs(arrays, str(tmp_path / "all"))
    for name, arr in arrays.items():
        assert np.array_equal(np.load(tmp_path / "all" / f"{name}.npy"), arr)
    # over the bound: the large array becomes a fixed sample of its elements, the same on every call
    cap = 8000
    for d in ("s1", "s2"):
        bench.write_outputs(arrays, str(tmp_path / d), cap=cap)
    assert sorted(os.listdir(tmp_path / "s1")) == ["eval.0.big.sample.npy", "eval.0.small.npy"]
    s1, s2 = (np.load(tmp_path / d / "eval.0.big.sample.npy") for d in ("s1", "s2"))
    assert np.array_equal(s1, s2) and s1.size == cap // 2 // 4 and np.isin(s1, arrays["eval.0.big"]).all()
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) < cap + 2 * 256


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr
