"""Worker of tests/test_syncbn_rccl_gpu.py: ``DDP(force_comm=True)`` plus
``convert_sync_batchnorm(force=True)`` under a 1-RANK RCCL communicator, so the synchronized
BatchNorm kernels and their collectives (on a process group of their own) run on the one-GPU
box exactly as they do at eight ranks, minus the link traffic.  Prints one JSON line."""
import copy
import json
import os
import sys
import traceback
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def scenario():
    from dmlab.models import ResNet18
    from dmlab.nn import convert_sync_batchnorm, cross_entropy
    from dmlab.optim import SGD
    from dmlab.parallel import DDP

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    X = torch.rand(16, 3, 64, 64, generator=g).to(dev)
    Y = torch.randint(0, 10, (16,), generator=g).to(dev)
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

    ref, auto = clone("torch"), clone("torch")
    F.cross_entropy(ref(X).float(), Y).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        oc = auto(X)
    F.cross_entropy(oc.float(), Y).backward()
    want, rc = grads(ref), [_rel(a, b) for a, b in zip(grads(auto), grads(ref))]

    def steps(sync):
        model = clone()
        if sync:
            convert_sync_batchnorm(model, force=True)
            assert model.stem._sync_bn.group is not None
        ddp = DDP(model, force_comm=True)
        opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.05, momentum=0.9))
        first = None
        for _ in range(2):
            opt.zero_grad()
            cross_entropy(ddp(X), Y).backward()
            if first is None:
                first = grads(model)
            opt.step()
        torch.cuda.synchronize()
        return model, ddp, first

    _, ddp0, _ = steps(False)
    model, ddp1, got = steps(True)
    bad = [(i, rn, c) for i, (rn, c) in
           enumerate(zip([_rel(a, b) for a, b in zip(got, want)], rc)) if rn > 1.5 * c + 0.05]
    return dict(ok=not bad, bad=bad, collectives=model.sync_bn_collectives,
                launched=ddp1.buckets_launched, launched_plain=ddp0.buckets_launched,
                finite=bool(torch.isfinite(model.flat.data).all().item()))


def main():
    from dmlab.parallel import env

    out = {}
    try:
        env.init(backend="nccl", timeout_s=120)
        assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
        out.update(scenario())
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
