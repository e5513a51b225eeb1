"""Host logic of bench.py that needs no GPU: `--dump-outputs` (bench.dump_outputs) on a small CPU model."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _model_after_a_step():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 2), torch.nn.Linear(2, 2))
    m[2].requires_grad_(False)       # a parameter that gets no gradient is dumped as zeros
    loss = m(torch.randn(4, 6)).square().mean()
    loss.backward()
    return m, loss


def test_dump_outputs_writes_the_loss_parameters_and_gradients_of_the_step(tmp_path):
    m, loss = _model_after_a_step()
    shapes = bench.dump_outputs(str(tmp_path / "out"), m, loss)
    n = sum(p.numel() for p in m.parameters())
    assert shapes == {"loss": (1,), "parameters": (n,), "gradients": (n,)}
    got = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in shapes}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"][0] == np.float32(loss.item())
    ps = list(m.parameters())
    assert np.array_equal(got["parameters"], torch.cat([p.detach().reshape(-1) for p in ps]).numpy())
    want_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps]).numpy()
    assert np.array_equal(got["gradients"], want_g)
    assert not got["gradients"][-6:].any() and got["gradients"][:-6].any()
    shapes = bench.dump_outputs(str(tmp_path / "nograds"), m, loss, with_grads=False)
    assert set(shapes) == {"loss", "parameters"} and sorted(os.listdir(tmp_path / "nograds")) == ["loss.npy", "parameters.npy"]


def test_dump_outputs_over_the_budget_is_the_same_seeded_sample_of_both_vectors(tmp_path, monkeypatch):
    m, loss = _model_after_a_step()
    n = sum(p.numel() for p in m.parameters())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096 + 2 * 4 * 20)      # 20 elements per vector
    full_p = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    full_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in m.parameters()]).numpy()
    for run in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / run), m, loss) == {"loss": (1,), "parameters": (20,), "gradients": (20,)}
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:20].sort().values.numpy()
    for k, full in (("parameters", full_p), ("gradients", full_g)):
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b) and np.array_equal(a, full[idx])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BUDGET_BYTES


def test_bench_options_without_a_gpu():
    """`--full` and `--dump-outputs` are options of the script; `--steps` below 1 is refused before anything runs."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr and out.stdout == ""
