"""bench.py's command line: a plain run reports the headline figure only,
`--full` adds the measurements that take runs of their own, and
`--dump-outputs DIR` writes what the last timed step computed as float32
.npy files (at most 64 MB; a fixed seeded sample of a larger output)."""
import json
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_files_and_fixed_sample(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8))
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    out = SimpleNamespace(loss=torch.tensor([1.5, 1.0, 0.5, 3.0]))
    bench.dump_outputs(str(tmp_path / "a"), out, model)
    got = {p.name: np.load(p) for p in sorted((tmp_path / "a").iterdir())}
    assert sorted(got) == ["bn_running_stats.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["loss.npy"], np.float32([1.5, 1.0, 0.5, 3.0]))
    assert np.array_equal(got["params.npy"], flat)
    # running_mean + running_var; the integer num_batches_tracked is left out
    assert got["bn_running_stats.npy"].shape == (16,)
    # above the cap: the same sampled positions on every call, in order
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), out, model, max_elems=50)
    b, c = np.load(tmp_path / "b/params.npy"), np.load(tmp_path / "c/params.npy")
    assert b.shape == (50,) and np.array_equal(b, c)
    idx = torch.randperm(flat.size, generator=torch.Generator().manual_seed(20))[:50].sort().values.numpy()
    assert np.array_equal(b, flat[idx])


@pytest.mark.gpu
def test_plain_bench_line_and_dump(dev, tmp_path):
    """One short plain run in a fresh process: the headline keys, nothing of
    `--full` measured, `--steps` reported as given, and the dump finite,
    float32 and within 64 MB."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - 256 / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
    assert line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["step_boundary"] is None
    files = sorted((tmp_path / "d").iterdir())
    assert [f.name for f in files] == ["bn_running_stats.npy", "loss.npy", "params.npy"]
    arrays = [np.load(f) for f in files]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays)
    assert sum(a.nbytes for a in arrays) <= 64 << 20
    assert np.allclose(arrays[1], line["last_loss"], atol=1e-5, rtol=0)
