"""Synchronized BatchNorm on the native kernels: two ranks sharing the box's single GPU (gloo),
ResNet-18 under DDP, against one fp32 process on the whole batch
(tests/syncbn_two_rank_worker.py)."""
import pytest

from dist_helpers import free_port

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stem_fused", ["1", "0"])
def test_resnet18_two_ranks_sync_bn(stem_fused):
    """32 images of 64 x 64, 16 per rank, two SGD steps.  After step 1 the DDP-averaged native
    gradient is held to the project's bound against the fp32 torch path on all 32 images
    (rn <= 1.5 * rc + 0.05 per parameter, rc = bf16 autocast on all 32); plain DDP, per-shard
    statistics, violates it for at least half of the parameters.  stem_fused 0: the
    space-to-depth stem, whose synced backward is the unfused mode 3."""
    import torch.multiprocessing as mp

    import syncbn_two_rank_worker as worker

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    port = free_port()
    ps = [ctx.Process(target=worker.entry, args=(r, 2, port, stem_fused, q)) for r in range(2)]
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
        print(rank, out)
        assert out["layers"] == 20 and out["params"] == 62
        assert not out["bad"], out["bad"]
        assert 2 * out["plain_bad"] >= out["params"], out
        assert out["stats_equal_step1"] and out["stats_equal_step2"]
        assert not out["stat_bad"], out["stat_bad"]
        assert out["collectives_step1"] == 40 and out["collectives"] == 80
        assert out["loss_finite"]
