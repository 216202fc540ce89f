"""Worker of tests/test_syncbn_multiproc_gpu.py: one of two ranks sharing the box's single
GPU (gloo group), ResNet-18 on the native kernels under DDP with synchronized BatchNorm."""
import copy
import os
import sys
import traceback
from pathlib import Path


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _run(rank, ws):
    import torch
    import torch.distributed as dist
    import torch.nn.functional as F

    from dmlab.models import ResNet18
    from dmlab.nn import ConvBN, convert_sync_batchnorm, cross_entropy
    from dmlab.optim import SGD
    from dmlab.parallel import DDP

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    X = torch.rand(32, 3, 64, 64, generator=g).to(dev)
    Y = torch.randint(0, 10, (32,), generator=g).to(dev)
    xs, ys = X[rank * 16:(rank + 1) * 16], Y[rank * 16:(rank + 1) * 16]
    torch.manual_seed(0)
    base = ResNet18(num_classes=10).to(dev)

    def clone(backend=None):
        m = copy.deepcopy(base)
        if backend:
            m.set_backend(backend)
        m._flatten()
        return m

    def grads(m):
        return [m.flat.grad_view(i).clone() for i in range(len(m.flat.params))]

    def bns(m):
        return [b for x in m.modules() if isinstance(x, ConvBN)
                for b in (x.running_mean, x.running_var)]

    # the yardsticks, on all 32 images: fp32 torch path, and bf16 autocast of it
    ref, auto = clone("torch"), clone("torch")
    F.cross_entropy(ref(X).float(), Y).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        oc = auto(X)
    F.cross_entropy(oc.float(), Y).backward()
    want, rc = grads(ref), [_rel(a, b) for a, b in zip(grads(auto), grads(ref))]

    def violations(got):
        return [(i, rn, c) for i, (rn, c) in
                enumerate(zip([_rel(a, b) for a, b in zip(got, want)], rc)) if rn > 1.5 * c + 0.05]

    # plain DDP: per-shard statistics, another model
    plain = clone()
    cross_entropy(DDP(plain, broadcast_buffers=False)(xs), ys).backward()
    plain_bad = len(violations(grads(plain)))

    model = clone()
    convert_sync_batchnorm(model)
    ddp = DDP(model, broadcast_buffers=False)
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9)
    out = {"plain_bad": plain_bad, "params": len(want), "layers": len(bns(model)) // 2}
    for step in range(2):
        opt.zero_grad()
        loss = cross_entropy(ddp(xs), ys)
        loss.backward()
        if step == 0:
            out["bad"] = violations(grads(model))
            out["collectives_step1"] = model.sync_bn_collectives
            # running statistics against the whole-batch fp32 run
            stat_bad = []
            for i, (a, b) in enumerate(zip(bns(model), bns(ref))):
                if not torch.allclose(a, b, rtol=2e-2, atol=2e-3):
                    stat_bad.append((i, float((a - b).abs().max())))
            out["stat_bad"] = stat_bad
        opt.step()
        # bit-equal across the ranks, with no buffer broadcast
        flat = torch.cat([b.reshape(-1) for b in bns(model)])
        both = [torch.empty_like(flat) for _ in range(ws)]
        dist.all_gather(both, flat)
        out[f"stats_equal_step{step + 1}"] = bool(torch.equal(both[0], both[1]))
    torch.cuda.synchronize()
    out["collectives"] = model.sync_bn_collectives
    out["loss_finite"] = bool(torch.isfinite(loss).item())
    return out


def entry(rank, ws, port, stem_fused, q):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(ws), LOCAL_RANK="0", DMLAB_STEM_FUSED=stem_fused)
    try:
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        res = _run(rank, ws)
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:
        q.put((rank, None, traceback.format_exc()))
