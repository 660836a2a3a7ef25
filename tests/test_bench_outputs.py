"""bench.py --dump-outputs on the CPU: the arrays a step leaves are named after their modules and
written as float32 .npy, and an output past the size limit is cut to the same seeded sample every time."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


class _Trainer:
    def __init__(self):
        self.sdf = torch.nn.Linear(3, 2)
        self.col = torch.nn.Linear(2, 1, bias=False)
        self.all_params = list(self.sdf.parameters()) + list(self.col.parameters())


def test_step_outputs_name_loss_parameters_and_gradients():
    import bench
    tr = _Trainer()
    loss = tr.col(tr.sdf(torch.ones(4, 3))).sum()
    loss.backward()
    out = bench.step_outputs(tr, loss)
    assert sorted(out) == ["grad.col.weight", "grad.sdf.bias", "grad.sdf.weight", "loss",
                           "param.col.weight", "param.sdf.bias", "param.sdf.weight"]
    assert out["param.sdf.weight"] is tr.sdf.weight and out["grad.sdf.weight"] is tr.sdf.weight.grad
    image = {"rgb": torch.zeros(2, 2, 3)}
    assert bench.step_outputs(tr, loss, image).keys() == image.keys()


def test_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    import bench
    big = torch.arange(10000, dtype=torch.float64).view(100, 100)
    tensors = {"big": big, "small": torch.tensor(1.5, requires_grad=True)}
    bench.dump_outputs(str(tmp_path / "a"), tensors)
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (100, 100) and np.array_equal(a, big.numpy())
    assert np.load(tmp_path / "a" / "small.npy") == np.float32(1.5)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    bench.dump_outputs(str(tmp_path / "b"), tensors)
    bench.dump_outputs(str(tmp_path / "c"), tensors)
    b, c = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (512,) and np.array_equal(b, c)
    assert np.all(np.diff(b) > 0) and set(b.tolist()) <= set(range(10000))  # a sample of big's own elements
    assert sorted(os.listdir(tmp_path / "b")) == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 4096 + 2 * 128
