"""Label-smoothed cross-entropy, EvalMetrics, ShardSampler and sharded evaluation on the CPU:
the torch fallbacks against the same references as the GPU kernels, the gloo all-reduce of
the metric state, and the task3 flags end to end."""
import json
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from dist_helpers import free_port, run_dist
from loss_metrics_ref import (SHAPES, assert_mixed, planted_labels, ref_counts, ref_nll_sum)

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------ loss
@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("B,C", SHAPES)
def test_smoothed_cross_entropy_cpu(B, C, eps):
    from dmlab.nn import CrossEntropyLoss, cross_entropy

    g = torch.Generator().manual_seed(B * 1000 + C)
    x = (torch.randn(B, C, generator=g) * 3).requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=g)
    l1 = cross_entropy(x, y, label_smoothing=eps)
    l1.backward(torch.tensor(2.0))
    xr = x.detach().double().requires_grad_(True)
    l2 = F.cross_entropy(xr, y, label_smoothing=eps)
    (2 * l2).backward()
    torch.testing.assert_close(l1, l2.float(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(x.grad, xr.grad.float(), rtol=1e-6, atol=1e-6)
    assert torch.equal(CrossEntropyLoss(label_smoothing=eps)(x.detach(), y), l1.detach())
    # the closed forms the kernels implement
    xd = x.detach().double()
    lse = torch.logsumexp(xd, 1)
    row = (1 - eps) * (lse - xd.gather(1, y[:, None])[:, 0]) + eps * (lse - xd.mean(1))
    assert abs(row.mean().item() - l2.item()) < 1e-12 * max(1.0, abs(l2.item()))


@pytest.mark.parametrize("eps", [-0.1, 1.5])
def test_label_smoothing_out_of_range(eps):
    from dmlab.nn import CrossEntropyLoss, cross_entropy

    x, y = torch.zeros(2, 3), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError):
        cross_entropy(x, y, label_smoothing=eps)
    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=eps)


# ------------------------------------------------------------------ metrics
def _ks(B, C):
    return [k for k in (1, 5, C, C + 3) if k != 1 or B >= 5]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", SHAPES)
def test_eval_metrics_cpu(B, C, dtype):
    from dmlab.nn import EvalMetrics

    g = torch.Generator().manual_seed(B + C)
    x = (torch.randn(B, C, generator=g) * 3).to(dtype)
    # one row cannot both hit and miss: B = 1 runs the two plantings (rank 0 and rank 5)
    for shift in ((0, 1) if B == 1 else (0,)):
        y = planted_labels(x, shift)
        for k in _ks(B, C):
            if k < C and B >= 5:
                assert_mixed(x, y, k)
            r = EvalMetrics(k=k).update(x, y).result()
            assert [r["n"], r["top1"], r["topk"]] == ref_counts(x, y, k)
            assert r["k"] == k
            ref = ref_nll_sum(x, y).item() / B
            assert abs(r["loss"] - ref) <= 1e-4 + 1e-4 * abs(ref)
    if B == 1:
        hit = [EvalMetrics(k=5).update(x, planted_labels(x, s)).result()["topk"] for s in (0, 1)]
        assert hit == [1, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C", [(6, 65), (300, 1000)])
def test_eval_metrics_ties_cpu(B, C, dtype):
    from dmlab.nn import EvalMetrics

    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (B, C), generator=g).to(dtype)
    y = planted_labels(x, mult=2)
    same = x.float() == x.float().gather(1, y[:, None])
    assert bool((same.sum(1) >= 2).all())  # every label sits inside a tie group
    for k in (1, 5, C, C + 3):
        r = EvalMetrics(k=k).update(x, y).result()
        assert [r["n"], r["top1"], r["topk"]] == ref_counts(x, y, k)


def test_eval_metrics_guards_and_accumulation_cpu():
    from dmlab.nn import EvalMetrics, count_correct

    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 10, generator=g) * 3
    y = planted_labels(x)
    m = EvalMetrics(k=5)
    m.update(x, y).update(x[:5], y[:5])
    a, b = ref_counts(x, y, 5), ref_counts(x[:5], y[:5], 5)
    r = m.result()
    assert [r["n"], r["top1"], r["topk"]] == [a[i] + b[i] for i in range(3)]
    assert r["top1"] == int(count_correct(x, y)) + int(count_correct(x[:5], y[:5]))
    # out-of-range labels: a miss with loss 0; a NaN label logit: a miss
    xb = x.clone()
    yb = y.clone()
    yb[0], yb[1] = -1, 10
    xb[2, yb[2]] = float("nan")
    r = EvalMetrics(k=13).update(xb, yb).result()
    assert r["n"] == 8 and r["topk"] == 5
    r = EvalMetrics(k=13).update(xb[:2], yb[:2]).result()
    assert r == {"n": 2, "top1": 0, "topk": 0, "k": 13, "loss": 0.0}
    with pytest.raises(ValueError):
        EvalMetrics(k=0)
    assert EvalMetrics(k=2).all_reduce().result()["n"] == 0  # no process group: a no-op


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("ws", [1, 2, 3, 8])
def test_shard_sampler(ws):
    from dmlab.data import DeviceLoader, ShardSampler, TensorDataset

    N = 101
    ds = TensorDataset(torch.arange(N).float()[:, None], torch.arange(N))
    shards = [ShardSampler(ds, ws, r) for r in range(ws)]
    idx = [s.indices().tolist() for s in shards]
    assert [len(s) for s in shards] == [len(i) for i in idx]
    assert [list(s) for s in shards] == idx
    assert sum(len(i) for i in idx) == N  # not padded
    assert sorted(sum(idx, [])) == list(range(N))  # disjoint and complete
    assert all(i == list(range(r, N, ws)) for r, i in enumerate(idx))
    seen = [int(v) for r in range(ws) for _, lab in DeviceLoader(ds, 16, sampler=shards[r])
            for v in lab]
    assert sorted(seen) == list(range(N))
    with pytest.raises(ValueError):
        ShardSampler(ds, 2, 2)


# ------------------------------------------------------------------ sharded evaluation
def _table(N=101, C=16):
    from dmlab.data import TensorDataset

    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, generator=g) * 3
    return TensorDataset(x, planted_labels(x))


def _single(k=5):
    from dmlab.data import DeviceLoader
    from dmlab.nn import EvalMetrics

    ds = _table()
    m = EvalMetrics(k=k)
    for x, y in DeviceLoader(ds, 16):
        m.update(x, y)
    return m


def _sharded_eval(rank, ws, _):
    from dmlab.data import DeviceLoader, ShardSampler
    from dmlab.nn import EvalMetrics
    from dmlab.tasks.common import evaluate

    ds = _table()
    ref = _single()
    m = EvalMetrics(k=5)
    loader = DeviceLoader(ds, 16, sampler=ShardSampler(ds, ws, rank))
    for x, y in loader:
        m.update(x, y)
    assert int(m.counts[0]) == len(range(rank, len(ds), ws))
    m.all_reduce()
    assert torch.equal(m.counts, ref.counts), (rank, m.counts, ref.counts)
    a, b = m.loss_sum.item(), ref.loss_sum.item()
    assert abs(a - b) <= 1e-12 * abs(b), (rank, a, b)
    lines = []
    ev = evaluate(torch.nn.Identity(), loader, k=5, sharded=True, print_fn=lines.append)
    rr = ref.result()
    assert ev["eval_samples"] == len(ds) == rr["n"]
    assert ev["top1"] == rr["top1"] / len(ds) and ev["topk"] == rr["topk"] / len(ds)
    assert (len(lines) == 3) == (rank == 0) and (rank == 0 or not lines)


@pytest.mark.slow
@pytest.mark.parametrize("ws", [2, 3])
def test_sharded_evaluation_gloo(ws):
    ref = _single().result()
    assert 0 < ref["top1"] < ref["topk"] < ref["n"] == 101
    run_dist(_sharded_eval, ws, None)


def test_evaluate_prints_reference_line_plus_one():
    from dmlab.data import DeviceLoader
    from dmlab.tasks.common import evaluate, test as run_test

    ds = _table()
    model = torch.nn.Identity()
    old, new = [], []
    acc = run_test(model, DeviceLoader(ds, 16), print_fn=old.append)
    ev = evaluate(model, DeviceLoader(ds, 16), k=5, print_fn=new.append)
    assert new[:len(old)] == old and len(new) == len(old) + 1
    assert re.fullmatch(r"\nTest set: Accuracy: \d+/101 \(\d+\.\d{2}%\)\n", new[-2])
    r = _single().result()
    assert new[-1] == "Test set: Top-5: {}/101 ({:.2f}%), loss: {:.4f}".format(
        r["topk"], 100 * r["topk"] / 101, r["loss"])
    assert ev["top1"] == acc and ev["eval_samples"] == 101 and ev["k"] == 5
    assert model.training


# ------------------------------------------------------------------ task3
NEW_KEYS = ("top1", "topk", "k", "test_loss", "eval_samples", "label_smoothing")


def _task3(extra, tmp_path, nproc=2):
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2")
    js = tmp_path / "r.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m",
           "dmlab.tasks.task3", "--device", "cpu", "--synthetic", "--train-samples", "2560",
           "--epochs", "1", "--lr", "0.01", "--json", str(js)] + extra
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    return r, js


@pytest.mark.slow
def test_task3_label_smoothing_topk_sharded(tmp_path):
    r, js = _task3(["--label-smoothing", "0.1", "--topk", "5", "--eval", "sharded"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    s = json.loads(js.read_text())
    assert all(k in s for k in NEW_KEYS)
    assert s["eval_samples"] == 10000  # the whole synthetic test set, nothing counted twice
    assert 0 <= s["top1"] <= s["topk"] <= 1 and s["accuracy"] == s["top1"]
    assert s["k"] == 5 and s["label_smoothing"] == 0.1 and math.isfinite(s["test_loss"])
    losses = [float(v) for v in re.findall(r"loss: (\d+\.\d+)", r.stdout)]
    assert losses and all(math.isfinite(v) for v in losses)
    assert len(re.findall(r"Test set: Accuracy: \d+/10000 \(\d+\.\d{2}%\)", r.stdout)) == 1
    assert len(re.findall(r"Test set: Top-5: \d+/10000", r.stdout)) == 1


@pytest.mark.slow
def test_task3_default_flags_unchanged(tmp_path):
    r, js = _task3([], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    s = json.loads(js.read_text())
    assert not [k for k in NEW_KEYS if k in s] and "accuracy" in s
    assert "Test set: Accuracy" in r.stdout and "Top-" not in r.stdout


def test_task3_fused_rejects_label_smoothing(tmp_path):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "dmlab.tasks.task3", "--device", "cpu", "--synthetic",
                        "--fused", "1", "--label-smoothing", "0.1"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--label-smoothing needs the layer-wise loop" in r.stderr
