"""CPU: bench.py's --dump-outputs writer (the whole output within 64 MB, a seeded sample with its flat indices above it) and the
options a plain run and a --full run are told apart by."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_the_whole_output_within_the_budget(tmp_path):
    import bench
    x = torch.randn(4, 400, 64, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(str(tmp_path / "d"), "latents", x.to(torch.bfloat16))
    assert sorted(os.listdir(tmp_path / "d")) == ["latents.npy"]
    got = np.load(tmp_path / "d" / "latents.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.to(torch.bfloat16).float().numpy())
    bench.dump_outputs(str(tmp_path / "e"), "latents", x.double())
    assert np.load(tmp_path / "e" / "latents.npy").dtype == np.float64


def test_dump_outputs_samples_a_larger_output_with_a_fixed_seed(tmp_path):
    import bench
    x = torch.arange(17 << 20, dtype=torch.float32).reshape(17, 1024, 1024)       # 68 MB: above the budget
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "vertices", x)
        assert sorted(os.listdir(tmp_path / d)) == ["vertices.npy", "vertices_index.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= bench.DUMP_LIMIT
    vals, idx = np.load(tmp_path / "a" / "vertices.npy"), np.load(tmp_path / "a" / "vertices_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and vals.shape == idx.shape and len(idx) > 1_000_000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < x.numel()
    assert np.array_equal(vals, x.reshape(-1).numpy()[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "vertices_index.npy"))      # the same sample from run to run
    assert np.array_equal(vals, np.load(tmp_path / "b" / "vertices.npy"))


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout and "--steps" in r.stdout
