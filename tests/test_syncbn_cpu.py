"""Synchronized BatchNorm on the CPU (gloo): the torch path of ConvBN against one process
on the concatenated batch, at the layer (float64, unequal shards) and the model level
(ResNet-18 fp32 under DDP), and the public interface (convert_sync_batchnorm, task3)."""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from dist_helpers import free_port, run_dist

ROOT = Path(__file__).resolve().parent.parent


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


# ------------------------------------------------------------------ 1. layer level
def _layer_worker(rank, ws, shards):
    import torch.distributed as dist

    from dmlab.nn import ConvBN, convert_sync_batchnorm

    C, n = 8, sum(shards)
    g = torch.Generator().manual_seed(11)
    X = torch.randn(n, 3, 6, 6, generator=g, dtype=torch.float64)
    Wt = torch.randn(n, C, 6, 6, generator=g, dtype=torch.float64)  # loss = Σ out * Wt
    torch.manual_seed(0)
    ref = ConvBN(3, C, 3, 1, 1, relu=True).double()
    with torch.no_grad():
        ref.bn_weight.copy_(torch.rand(C, dtype=torch.float64) + 0.5)
        ref.bn_bias.copy_(torch.randn(C, dtype=torch.float64))
    layer = copy.deepcopy(ref)
    assert convert_sync_batchnorm(layer) is layer and layer._sync_bn is not None
    # one process, the concatenated batch
    xr = X.clone().requires_grad_(True)
    out_ref = ref(xr)
    (out_ref * Wt).sum().backward()
    # this rank's shard; the sum of the per-rank losses is the whole-batch objective
    lo = sum(shards[:rank])
    hi = lo + shards[rank]
    xs = X[lo:hi].clone().requires_grad_(True)
    out = layer(xs)
    (out * Wt[lo:hi]).sum().backward()
    tol = dict(rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(out, out_ref[lo:hi], **tol)
    torch.testing.assert_close(xs.grad, xr.grad[lo:hi], **tol)
    for name in ("weight", "bn_weight", "bn_bias"):
        gsum = getattr(layer, name).grad.clone()
        dist.all_reduce(gsum)  # DDP's average times ws: the whole-batch gradient
        torch.testing.assert_close(gsum / ws, getattr(ref, name).grad / ws, **tol)
    torch.testing.assert_close(layer.running_mean, ref.running_mean, **tol)
    torch.testing.assert_close(layer.running_var, ref.running_var, **tol)
    assert int(layer.num_batches_tracked) == 1
    assert layer._sync_bn_state.collectives == 2  # one all-gather, one all-reduce
    # eval mode: running statistics, no collective
    layer.eval()
    ref.eval()
    torch.testing.assert_close(layer(X[:2]), ref(X[:2]), **tol)
    assert layer._sync_bn_state.collectives == 2


@pytest.mark.parametrize("shards", [(5, 3), (4, 3, 1)])
def test_layer_matches_whole_batch_float64(shards):
    run_dist(_layer_worker, len(shards), shards)


# ------------------------------------------------------------------ 2. model level
def _model_grads(model, ddp, X, Y, rank):
    from dmlab.nn import cross_entropy

    model.flat.grad.zero_()
    cross_entropy(ddp(X[rank * 8:(rank + 1) * 8]), Y[rank * 8:(rank + 1) * 8]).backward()
    return [model.flat.grad_view(i).clone() for i in range(len(model.flat.params))]


def _model_worker(rank, ws):
    import torch.distributed as dist

    from dmlab.models import ResNet18
    from dmlab.nn import ConvBN, convert_sync_batchnorm, cross_entropy
    from dmlab.parallel import DDP

    # Data seed: a random-initialised ResNet has discrete events (ReLU / max-pool decisions
    # on near-ties) that fp32 rounding alone can flip.  For about half of the data seeds the
    # fp32 whole-batch reference ITSELF is then 4e-3 .. 1.3e-2 away from its float64 evaluation
    # in the layer-1 and stem gradients (seeds 7, 2, 5), for the others 6e-6 (seeds 1, 3, 11).
    # The 1e-4 bound needs a reference that is good to 1e-4, so the seed is one of the latter.
    g = torch.Generator().manual_seed(1)
    X = torch.rand(16, 3, 32, 32, generator=g)
    Y = torch.randint(0, 10, (16,), generator=g)
    torch.manual_seed(0)
    base = ResNet18(num_classes=10)
    ref = copy.deepcopy(base)
    ref._flatten()
    cross_entropy(ref(X), Y).backward()
    want = [ref.flat.grad_view(i).clone() for i in range(len(ref.flat.params))]

    plain = copy.deepcopy(base)
    plain._flatten()
    got_plain = _model_grads(plain, DDP(plain, broadcast_buffers=False), X, Y, rank)
    missed = sum(_rel(a, b) >= 1e-4 for a, b in zip(got_plain, want))
    assert 2 * missed >= len(want), (missed, len(want))  # per-shard BN is another model

    model = copy.deepcopy(base)
    model._flatten()
    convert_sync_batchnorm(model)
    got = _model_grads(model, DDP(model, broadcast_buffers=False), X, Y, rank)
    errs = {f"{i}:{n}": _rel(a, b) for i, (n, a, b) in enumerate(zip(model.flat.names, got, want))}
    print("syncbn model-level rel errors: max", max(errs.values()))
    bad = {n: e for n, e in errs.items() if not e < 1e-4}
    assert not bad, bad
    assert model.sync_bn_collectives == 40
    # running statistics: bit-equal across ranks without any broadcast
    for m in model.modules():
        if isinstance(m, ConvBN):
            for buf in (m.running_mean, m.running_var):
                both = [torch.empty_like(buf) for _ in range(ws)]
                dist.all_gather(both, buf)
                assert torch.equal(both[0], both[1])


def test_resnet18_ddp_matches_whole_batch_fp32():
    run_dist(_model_worker, 2)


# ------------------------------------------------------------------ 3. interface
def test_convert_without_group_is_noop():
    from dmlab.models import ResNet18
    from dmlab.nn import ConvBN, convert_sync_batchnorm

    torch.manual_seed(0)
    m = ResNet18(num_classes=10)
    assert convert_sync_batchnorm(m) is m
    assert all(x._sync_bn is None for x in m.modules() if isinstance(x, ConvBN))
    assert m.sync_bn_collectives == 0
    assert ResNet18(num_classes=10, sync_bn=True).stem._sync_bn is None
    # force: the sync arithmetic runs (one rank, no group, no collective)
    x = torch.rand(4, 3, 32, 32)
    want = m(x)
    f = convert_sync_batchnorm(copy.deepcopy(m), force=True)
    f._flatten()
    assert f.stem._sync_bn is not None
    got = f(x)
    assert _rel(got, want) < 1e-4 and f.sync_bn_collectives == 0


def test_task3_sync_bn_needs_resnet(capsys):
    from dmlab.tasks import task3

    with pytest.raises(SystemExit) as e:
        task3.parse_args(["--sync-bn", "on", "--model", "lenet"])
    assert e.value.code == 2 and "--sync-bn" in capsys.readouterr().err
    assert task3.parse_args([]).sync_bn == "off"


def test_task3_two_ranks_sync_bn(tmp_path):
    env = dict(os.environ, PYTHONPATH=str(ROOT), OMP_NUM_THREADS="2")
    js = tmp_path / "r.json"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), "-m",
           "dmlab.tasks.task3", "--model", "resnet18", "--device", "cpu", "--sync-bn", "on",
           "--max-steps", "2", "--synthetic", "--train-samples", "64", "--batch-size", "4",
           "--image-size", "32", "--epochs", "1", "--no-test", "--json", str(js)]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    s = json.loads(js.read_text())
    assert s["sync_bn"] == "on" and s["steps"] == 2
    assert s["sync_bn_collectives"] == 2 * 40
