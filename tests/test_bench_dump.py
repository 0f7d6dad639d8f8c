"""CPU: bench.py --dump-outputs writes what the timed step returns (logits, loss, gradients) as float .npy files, within its size
budget, and the gradient sample sits at the same positions in every run; --steps below 1 is refused before any GPU work."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _model_with_grads(seed):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.GELU(), torch.nn.Linear(32, 2))
    x = torch.randn(5, 16, generator=torch.Generator().manual_seed(1))
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, torch.tensor([0, 1, 1, 0, 1]))
    loss.backward()
    return model, logits, loss


def test_dump_writes_float_arrays_of_the_last_step(tmp_path):
    model, logits, loss = _model_with_grads(0)
    named = list(model.named_parameters())
    bench.dump_outputs(str(tmp_path), logits, loss, named)
    files = sorted(os.listdir(tmp_path))
    assert files == ["grad_norms.npy", "grad_sample.npy", "logits.npy", "loss.npy"]
    arrays = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert np.array_equal(arrays["logits"], logits.detach().numpy()) and arrays["loss"] == np.float32(loss.item())
    assert np.allclose(arrays["grad_norms"], [float(p.grad.double().norm()) for _, p in named])
    # everything fits the sample budget here: the gradients are dumped whole, in named_parameters() order
    assert np.array_equal(arrays["grad_sample"], torch.cat([p.grad.reshape(-1) for _, p in named]).numpy())


def test_dump_samples_large_gradients_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_GRAD_SAMPLE", 100)
    model, logits, loss = _model_with_grads(0)
    named = list(model.named_parameters())
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), logits, loss, named)
    a, b = np.load(tmp_path / "a" / "grad_sample.npy"), np.load(tmp_path / "b" / "grad_sample.npy")
    assert a.shape == (100,) and a.dtype == np.float32 and np.array_equal(a, b)
    flat = torch.cat([p.grad.reshape(-1) for _, p in named]).numpy()
    assert np.isin(a, flat).all()


def test_default_budget_stays_under_64_mb():
    assert bench.DUMP_GRAD_SAMPLE * 4 < 60 * 2**20


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
