"""bench.py's plain run and --dump-outputs: the line a plain run prints, the arrays the last timed step computed, and the
fixed sample that stands for an array too large to write whole."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_a_fixed_bounded_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_ELEMS_PER_ARRAY", 1000)
    g = torch.Generator().manual_seed(0)
    arrays = {"rows": torch.randn(500, 128, generator=g), "flat": torch.randn(5000, generator=g),
              "small": torch.randn(7, 3, generator=g, dtype=torch.float64), "whole": torch.randn(10, 4, 2, generator=g)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b), name                                  # the same positions every time
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.shape == (1000 // 128, 128) and rows.dtype == np.float32
    src = arrays["rows"].numpy()
    picked = [int(np.flatnonzero((src == r).all(axis=1))[0]) for r in rows]
    assert picked == sorted(set(picked))                                  # whole rows of the array, in ascending order
    flat = np.load(tmp_path / "a" / "flat.npy")
    assert flat.shape == (1000,) and np.isin(flat, arrays["flat"].numpy()).all()
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float64 and np.array_equal(small, arrays["small"].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "whole.npy"), arrays["whole"].numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), arrays)


def _plain_run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--graphs", "512", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    d = _plain_run(tmp_path / "a", 3)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["unit"] == "edges/s"
    assert d["metric"].startswith("edges/sec through one CGAT attention layer") and d["dtype"].startswith("f32 storage")
    assert abs(d["value"] - d["config"]["edges_per_rank"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"cpu_baseline", "modes", "roofline", "kernel_ms_per_step"} & set(d)      # those are --full's
    E = d["config"]["edges_per_rank"]
    N = E // 12
    shapes = {"out": (N, 128), "grad_x": (N, 128), "grad_x0": (N, 128), "grad_edge_attr": ((1 << 21) // 128, 128),
              "grad_params": (1 << 21,)}
    total = 0
    for name, shape in shapes.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.shape == shape and a.dtype == np.float32 and np.isfinite(a).all(), (name, a.shape, a.dtype)
        total += a.nbytes
    assert total <= 64_000_000
    # another step count over the same inputs and parameters: the same last step, up to the order of floating-point sums
    _plain_run(tmp_path / "b", 2)
    for name in shapes:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.abs(a - b).max() <= 1e-5 * max(np.abs(a).max(), 1e-30), name
