"""bench.py --dump-outputs / --steps: the result line of a plain run and the arrays it writes."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_fits_the_budget_and_samples_the_same_positions(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = {"x1_hat": torch.rand(8, 3, 1024, 1024, generator=g).half(), "y1_hat": torch.randn(8, 192, 32, 32, generator=g),
           "likelihoods": {"z1": torch.rand(8, 128, 8, 8, generator=g)}}
    rd = {"bits_z1": torch.full((1,), 3.5, dtype=torch.float64), "num_pixels": 8 * 1024 * 1024}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.flat_outputs(out, rd))
    names = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "a" / "*.npy")))
    assert names == ["likelihoods_z1.npy", "rd_bits_z1.npy", "x1_hat.npy", "y1_hat.npy"]
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 * 10 ** 6
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "rd_bits_z1.npy").dtype == np.float64
    y = np.load(tmp_path / "a" / "y1_hat.npy")
    assert y.shape == (8, 192, 32, 32) and np.array_equal(y, out["y1_hat"].numpy())          # small enough: written whole
    x = np.load(tmp_path / "a" / "x1_hat.npy")
    assert x.ndim == 1 and 0 < x.size < out["x1_hat"].numel()                                  # too large: a sample of its elements
    assert np.isin(x, out["x1_hat"].float().numpy().reshape(-1)).all()


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_asked_and_dumps_the_last_step(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2", "--size", "256",
           "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert d["roofline"] is None and d["cpu_baseline"] is None and "secondary" not in d
    files = {os.path.basename(f): np.load(f) for f in glob.glob(str(tmp_path / "out" / "*.npy"))}
    for k in ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "likelihoods_y1", "rd_sse1", "rd_sse2"):
        a = files[k + ".npy"]
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), k
    assert files["y1_hat.npy"].shape == (2, 192, 16, 16)
    assert np.array_equal(files["y1_hat.npy"], np.round(files["y1_hat.npy"]))                   # rounded latents
