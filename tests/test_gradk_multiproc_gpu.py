"""Two ranks sharing the box's single GPU over gloo (as tests/test_multiproc_gpu.py):
LeNet under DDP(compress='topk') for three steps.  Both ranks end with the same bits, and those
are the bits of a single-process simulation on the same device that computes each rank's
gradient and applies the codec by hand."""
import os

import pytest
import torch

from dist_helpers import free_port

pytestmark = pytest.mark.gpu
STEPS, PER, KEEP = 3, 8, 32


def _simulate(ws, bounds, X, Y, dev):
    from dmlab.models import Net
    from dmlab.nn import cross_entropy
    from dmlab.optim import SGD
    from dmlab.parallel.compress import TopKCompressor

    torch.manual_seed(0)
    model = Net().to(dev)
    opt = SGD(model.parameters(), lr=0.1, momentum=0.9)
    opt.grad_scale = 1.0 / ws  # the average folded into the optimiser, as the ranks do
    n = model.flat.grad.numel()
    comps = [TopKCompressor(n, dev, keep=KEEP) for _ in range(ws)]
    for _ in range(STEPS):
        grads = []
        for rk in range(ws):
            opt.zero_grad()
            cross_entropy(model(X[rk * PER:(rk + 1) * PER]), Y[rk * PER:(rk + 1) * PER]).backward()
            grads.append(model.flat.grad.clone())
        for lo, hi in bounds:
            rows = torch.zeros((ws, comps[0].payload_bytes(hi - lo)), dtype=torch.uint8, device=dev)
            for rk in range(ws):
                comps[rk].encode(grads[rk][lo:hi], lo, rows[rk])
            comps[0].decode_mean(rows, model.flat.grad[lo:hi], 1.0)
        opt.step()
    torch.cuda.synchronize()
    return model.flat.data.clone(), [c.residual.clone() for c in comps]


def _entry(rank, ws, port, q):
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(ws), LOCAL_RANK="0")
    import torch.distributed as dist

    try:
        from dmlab.models import Net
        from dmlab.nn import cross_entropy
        from dmlab.optim import SGD
        from dmlab.parallel import DDP

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
        g = torch.Generator().manual_seed(5)
        X = torch.rand(ws * PER, 1, 28, 28, generator=g).to(dev)
        Y = torch.randint(0, 10, (ws * PER,), generator=g).to(dev)
        torch.manual_seed(0)
        model = Net().to(dev)
        ddp = DDP(model, compress="topk", compress_keep=KEEP, bucket_cap_mb=0.05,
                  first_bucket_mb=0.01)
        assert ddp._native is None and len(ddp.buckets) >= 2
        opt = ddp.fold_average_into(SGD(model.parameters(), lr=0.1, momentum=0.9))
        for _ in range(STEPS):
            opt.zero_grad()
            cross_entropy(ddp(X[rank * PER:(rank + 1) * PER]), Y[rank * PER:(rank + 1) * PER]).backward()
            opt.step()
        torch.cuda.synchronize()
        assert ddp.buckets_launched == STEPS * len(ddp.buckets)
        mine = model.flat.data.clone()
        rows = [torch.empty_like(mine) for _ in range(ws)]
        dist.all_gather(rows, mine)
        ranks_equal = all(bool(torch.equal(r, rows[0])) for r in rows)
        want, res = _simulate(ws, [(b.lo, b.hi) for b in ddp.buckets], X, Y, dev)
        q.put((rank, dict(ranks_equal=ranks_equal, sim_equal=bool(torch.equal(mine, want)),
                          residual_equal=bool(torch.equal(ddp.compressor.residual, res[rank])),
                          residual_max=float(res[rank].abs().max()),
                          max_diff=float((mine - want).abs().max())), None))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, None, traceback.format_exc()))


def test_two_ranks_one_gpu_ddp_topk():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    ps = [ctx.Process(target=_entry, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(240)
    res = [q.get() for _ in range(2) if not q.empty()]
    for p in ps:
        if p.is_alive():
            p.kill()
    assert len(res) == 2, res
    for rank, out, tb in res:
        assert tb is None, tb
        assert out["ranks_equal"] and out["sim_equal"] and out["residual_equal"], (rank, out)
        assert out["residual_max"] > 0
