"""Worker for tests/test_gradk_rccl_gpu.py: one topk-compression scenario per process, under a
1-RANK RCCL (ProcessGroupNCCL) communicator on the box's single GPU, as
tests/gradq_one_rank_worker.py does for the q8 codec.  With ``force_comm`` the encode kernel,
the ``all_gather_into_tensor`` of every bucket's payload and the decode-mean kernel run exactly
as they do at eight ranks (minus the link traffic).

Prints one JSON line ``{"scenario": ..., "ok": bool, ...}``.
"""
import json
import os
import sys
import traceback
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

KEEP = 32


def _by_hand(comp, grad, bounds, scale=1.0):
    """Push a gradient buffer bucket by bucket through TopKCompressor encode + decode-mean (one
    rank), in place."""
    for lo, hi in bounds:
        payload = torch.zeros(comp.payload_bytes(hi - lo), dtype=torch.uint8, device=grad.device)
        comp.encode(grad[lo:hi], lo, payload)
        comp.decode_mean(payload.view(1, -1), grad[lo:hi], scale)


def scenario_resnet_topk():
    """ResNet-18 at 8x3x64x64 under DDP(force_comm, compress='topk'): after each of two steps
    the gradient buffer equals the no-communication run's gradient pushed through the codec by
    hand (step 2 with the carried residual), bit for bit; one gather per bucket and step."""
    from dmlab.models import ResNet18
    from dmlab.nn import cross_entropy
    from dmlab.optim import SGD
    from dmlab.parallel import DDP
    from dmlab.parallel.compress import TopKCompressor

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    X = torch.rand(8, 3, 64, 64, generator=g).to(dev)
    Y = torch.randint(0, 10, (8,), generator=g).to(dev)

    def run(compressed, bounds=None):
        torch.manual_seed(0)
        model = ResNet18(num_classes=10).to(dev)
        ddp = (DDP(model, force_comm=True, compress="topk", compress_keep=KEEP) if compressed
               else DDP(model))
        opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.1, momentum=0.9))
        comp = None if compressed else TopKCompressor(model.flat.grad.numel(), dev, keep=KEEP)
        grads = []
        for _ in range(2):
            opt.zero_grad()
            cross_entropy(ddp(X), Y).backward()
            if not compressed:
                _by_hand(comp, model.flat.grad, bounds)
            grads.append(model.flat.grad.clone())
            opt.step()
        torch.cuda.synchronize()
        res = (ddp.compressor if compressed else comp).residual.clone()
        return ddp, grads, res, model.flat.data.clone()

    ddp, g1, r1, p1 = run(True)
    assert ddp._native is None and ddp.side_stream_hooks and ddp.compressor is not None
    nb = len(ddp.buckets)
    _, g0, r0, p0 = run(False, [(b.lo, b.hi) for b in ddp.buckets])
    same = [bool(torch.equal(a, b)) for a, b in zip(g1, g0)]
    nonzero = float((g1[0] != 0).float().mean())
    return dict(ok=all(same) and torch.equal(r1, r0) and torch.equal(p1, p0)
                and float(r1.abs().max()) > 0,
                steps_equal=same, residual_equal=bool(torch.equal(r1, r0)), buckets=nb,
                launched=ddp.buckets_launched, expect_launched=2 * nb, nonzero_share=nonzero,
                bytes_per_step=ddp.comm_bytes_per_step, fp32_bytes=4 * ddp.grad_buf.numel())


def scenario_lenet_graph_topk():
    """The fused LeNet DDP step with compress='topk' (encode, RCCL all-gather, decode-mean, SGD)
    captured once in a hipGraph and replayed 3 times == the same steps run eagerly, bit for
    bit: parameters and residual."""
    from dmlab.models import Net
    from dmlab.models.lenet_fused import FusedLeNetStep
    from dmlab.optim import SGD
    from dmlab.parallel import DDP
    from dmlab.utils.graph import CapturedStep

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    X = torch.rand(32, 1, 28, 28, generator=g).to(dev)
    Y = torch.randint(0, 10, (32,), generator=g).to(dev)
    runs = []
    for captured in (False, True):
        torch.manual_seed(0)
        model = Net().to(dev)
        ddp = DDP(model, force_comm=True, compress="topk", compress_keep=KEEP,
                  bucket_cap_mb=0.05, first_bucket_mb=0.01)
        assert ddp._native is None and len(ddp.buckets) >= 2
        opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.1, momentum=0.9))
        step = FusedLeNetStep(model, opt, ddp=ddp)
        if captured:
            cap = CapturedStep(step, [X, Y], warmup=2, bind_inputs=True)  # 2 eager steps first
            for _ in range(3):
                cap(X, Y)
        else:
            for _ in range(5):
                step(X, Y)
        torch.cuda.synchronize()
        runs.append((model.flat.data.clone(), ddp.compressor.residual.clone(),
                     ddp.buckets_launched, len(ddp.buckets)))
    (p0, r0, l0, nb), (p1, r1, l1, _) = runs
    return dict(ok=torch.equal(p0, p1) and torch.equal(r0, r1) and float(r0.abs().max()) > 0,
                max_diff=float((p0 - p1).abs().max()), res_diff=float((r0 - r1).abs().max()),
                eager_launched=l0, graph_launched=l1, buckets=nb)


def scenario_aggregator_topk():
    """GradAggregator('allgather_topk', force=True) over RCCL at one rank: the gradient becomes
    the codec's round trip of the local one; timing and byte fields are there."""
    from dmlab.models import Net
    from dmlab.nn import cross_entropy
    from dmlab.parallel import comm
    from dmlab.parallel.compress import TopKCompressor, topk_payload_bytes

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = Net().to(dev)
    x = torch.rand(16, 1, 28, 28, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    cross_entropy(model(x), y).backward()
    n = model.flat.grad.numel()
    want = model.flat.grad.clone()
    comp = TopKCompressor(n, dev, keep=KEEP)
    agg = comm.GradAggregator(model, "allgather_topk", force=True, keep=KEEP)
    same = True
    for _ in range(3):
        _by_hand(comp, want, [(0, n)])
        agg()
        same &= bool(torch.equal(model.flat.grad, want))
    same &= bool(torch.equal(agg.compressor.residual, comp.residual))
    t = agg.comm_time
    return dict(ok=bool(same) and t > 0 and agg.calls == 3
                and agg.bytes_per_call == topk_payload_bytes(n, KEEP),
                comm_time=t, bytes_per_call=agg.bytes_per_call, fp32_bytes=4 * n,
                allreduce_bytes=comm.GradAggregator(model, "allreduce").bytes_per_call)


def main():
    name = sys.argv[1]
    from dmlab.parallel import env

    out = {"scenario": name}
    try:
        env.init(backend="nccl", timeout_s=120)
        assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
        out.update(globals()["scenario_" + name]())
    except Exception:
        out.update(ok=False, error=traceback.format_exc())
    finally:
        try:
            env.destroy()
        except Exception:
            pass
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    main()
