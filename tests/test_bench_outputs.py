"""bench.py --dump-outputs / --full: what a plain run writes and what it leaves out."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def test_dump_outputs_files_and_sample(tmp_path, monkeypatch):
    """loss and the flat parameters as float32; above the byte budget the parameters are a
    fixed sample in index order, the same from call to call."""
    import bench
    from dmlab.models import Net

    torch.manual_seed(0)
    m = Net()
    flat = m.flat.data.detach().float().reshape(-1).numpy()
    loss = torch.tensor(1.25, dtype=torch.bfloat16)
    bench.dump_outputs(tmp_path / "a", loss, m)
    lo, p = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "params.npy")
    assert lo.dtype == np.float32 and lo.shape == (1,) and lo[0] == 1.25
    assert p.dtype == np.float32 and np.array_equal(p, flat)

    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 1001)  # loss + 1000 parameters
    bench.dump_outputs(tmp_path / "b", loss, m)
    bench.dump_outputs(tmp_path / "c", loss, m)
    pb, pc = np.load(tmp_path / "b" / "params.npy"), np.load(tmp_path / "c" / "params.npy")
    assert pb.shape == (1000,) and np.array_equal(pb, pc)
    idx = np.sort(np.random.default_rng(0).choice(flat.size, size=1000, replace=False))
    assert np.array_equal(pb, flat[idx])


def test_full_is_off_by_default(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain run (small ResNet-18 config) prints the headline line without the --full
    extras and writes the last timed step's loss and updated parameters."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--res", "64", "--batch", "16",
                        "--dump-outputs", str(out)], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "samples/s"
    assert abs(res["value"] - 16 / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    assert not {"phases_ms", "param_checksum", "replicas_in_sync"} & set(res)
    assert sorted(p.name for p in out.iterdir()) == ["loss.npy", "params.npy"]
    lo, p = np.load(out / "loss.npy"), np.load(out / "params.npy")
    assert lo.dtype == np.float32 and p.dtype == np.float32
    assert round(float(lo[0]), 4) == res["final_loss"]
    assert p.size > 11_000_000 and np.isfinite(p).all() and np.abs(p).max() > 0
    assert lo.nbytes + p.nbytes <= 64e6
