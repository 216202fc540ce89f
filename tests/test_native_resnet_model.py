"""End-to-end native ResNet-18 (bf16 NHWC HIP kernels) vs the same Program on the
PyTorch fp32 reference path."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dmlab.models import ResNet18
from dmlab.nn import cross_entropy
from dmlab.nn.program import Program
from dmlab.ops._native import lib

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def test_resnet18_native_matches_reference(dev):
    """bf16 vs fp32 differences compound through 20 BN layers of a random-init net
    (early-layer grads differ by ~40% for ANY bf16 implementation), so the native
    path is held to the error level of PyTorch's own bf16 autocast on the same
    model and data: native error <= 1.5 x autocast error + 0.05, per parameter."""
    lib()
    torch.manual_seed(0)
    a = ResNet18(num_classes=10).to(dev)
    b = copy.deepcopy(a).set_backend("torch")
    b._flatten()
    c = copy.deepcopy(b)
    c._flatten()
    x = torch.rand(16, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (16,), device=dev)
    la = cross_entropy(a(x), y)
    lb = F.cross_entropy(b(x), y)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        oc = c(x)
    lc = F.cross_entropy(oc.float(), y)
    for l in (la, lb, lc):
        l.backward()
    assert abs(la.item() - lb.item()) < 5e-2 * max(1.0, abs(lb.item()))
    bad = []
    for (n, pa), (_, pb), (_, pc) in zip(a.named_parameters(), b.named_parameters(),
                                         c.named_parameters()):
        rn, rc = _rel(pa.grad, pb.grad), _rel(pc.grad, pb.grad)
        if rn > 1.5 * rc + 0.05:
            bad.append((n, rn, rc))
    assert not bad, bad
    # running statistics were updated like torch's
    torch.testing.assert_close(a.stem.running_mean, b.stem.running_mean, rtol=2e-2, atol=2e-3)


def test_resnet18_eval_mode(dev):
    """Eval mode uses running statistics; error held to the torch-autocast level."""
    torch.manual_seed(1)
    a = ResNet18(num_classes=10).to(dev)
    b = copy.deepcopy(a).set_backend("torch")
    b._flatten()
    x = torch.rand(8, 3, 32, 32, device=dev)
    for m in (a, b):
        m.train()
        for _ in range(3):
            m(x)  # populate running stats
        m.eval()
    torch.testing.assert_close(a.layer2_0.c1.running_var, b.layer2_0.c1.running_var,
                               rtol=5e-2, atol=1e-2)
    with torch.no_grad():
        ref = b(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            auto = b(x)
        assert _rel(a(x), ref) < 1.5 * _rel(auto, ref) + 0.02


@pytest.mark.parametrize("res", [64, 224])
def test_fused_stem_backward_matches_unfused(dev, res, monkeypatch):
    """The fused stem backward (conv_stem.hip: the BN-backward apply and max-pool gather
    computed inside the s2d weight gradient, dy never written) gives the same stem gradients
    as the generic path (quad-apply pass writing dy + igemm s2d weight gradient; same bf16 dy,
    fp32 sums in another order), and every other gradient bit for bit."""
    import dmlab.ops.convbn as cb

    monkeypatch.setenv("DMLAB_STEM_FUSED", "0")  # the space-to-depth stem path
    torch.manual_seed(3)
    a = ResNet18(num_classes=10).to(dev)
    x = torch.rand(4, 3, res, res, device=dev)
    y = torch.randint(0, 10, (4,), device=dev)
    grads = []
    for fused in (False, True):
        with monkeypatch.context() as mp:
            if not fused:
                mp.setattr(cb.lib(), "stem_bwd_fused_supported", lambda *args: False)
            a.flat.grad.zero_()
            cross_entropy(a(x), y).backward()
            torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in a.named_parameters()})
    for n in grads[0]:
        if n.startswith("stem."):
            assert _rel(grads[1][n], grads[0][n]) < 2e-3, n
        else:
            torch.testing.assert_close(grads[1][n], grads[0][n], rtol=0, atol=0, msg=n)


def test_grad_hooks_see_final_wgrads(dev):
    """Each layer's grad hook (DDP's bucket launch point) runs after that layer's side-stream
    weight gradients: the snapshot it takes is the final gradient, bit for bit."""
    torch.manual_seed(5)
    a = ResNet18(num_classes=10).to(dev)
    x = torch.rand(8, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)
    snaps = {}

    def hook(prog, i):
        snaps[i] = [p.grad.detach().clone() for p in prog.layers[i].parameters()]

    a.register_grad_hook(hook)
    try:
        a.flat.grad.zero_()
        cross_entropy(a(x), y).backward()
        torch.cuda.synchronize()
    finally:
        a.remove_grad_hook(hook)
    assert sorted(snaps) == list(range(len(a.layers)))
    g = {n: p.grad.detach().clone() for n, p in a.named_parameters()}
    for i in snaps:
        for u, p in zip(snaps[i], a.layers[i].parameters()):
            torch.testing.assert_close(u, g[[n for n, q in a.named_parameters() if q is p][0]],
                                       rtol=0, atol=0)


def test_resnet18_training_trajectory_224(dev):
    """Ten SGD-momentum steps at the headline image shape (224 x 224, 1000 classes; batch
    32): the native kernels (res64 / pipe / halo / stem dispatch, fused dgrad-epilogue BN
    reductions, side-stream weight gradients) track the fp32 PyTorch run as closely as stock
    bf16 autocast does (tools/numerics_resnet.py; the long runs at batch 256 / 1024 are in
    profiles/numerics_resnet18_224_*.jsonl)."""
    from tools.numerics_resnet import run, summarize

    models, hist = run(32, 10, 224, nbatches=2, log=lambda s: None)
    s = summarize(models, hist)
    assert all(h["native"] == h["native"] for h in hist)  # finite
    assert s["max_loss_dist_native_fp32"] <= 2.0 * s["max_loss_dist_autocast_fp32"] + 0.05, s
    med = s["gnorm_rel_err_median"]
    assert med["native"] <= 2.0 * med["autocast"] + 0.1, s
    bn = s["bn_running_rel_err_max"]
    assert bn["native"] <= 2.0 * bn["autocast"] + 0.05, s


def test_resnet18_aux_stream_bit_identical(dev, monkeypatch):
    """The projection shortcuts' BN backward on the aux stream (BasicBlock.native_bwd,
    convbn_bwd phase 1/2) computes exactly what the serial order does: every gradient and
    running statistic bit-identical, over two steps so that stream-ordered memory reuse
    between steps is exercised too."""
    torch.manual_seed(5)
    base = ResNet18(num_classes=10).to(dev)
    x = torch.rand(8, 3, 64, 64, device=dev)
    y = torch.randint(0, 10, (8,), device=dev)
    grads, stats = {}, {}
    for aux in ("1", "0"):
        with monkeypatch.context() as mp:  # undone after each run: the order does not matter
            if aux == "0":  # the serial order: no aux stream
                mp.setattr(Program, "_aux_stream", lambda self: None)
            m = copy.deepcopy(base)
            for _ in range(2):
                m.zero_grad()
                cross_entropy(m(x), y).backward()
            torch.cuda.synchronize()
        grads[aux] = [p.grad.clone() for p in m.parameters()]
        stats[aux] = [b.clone() for b in m.buffers()]
    for ga, gb in zip(grads["1"], grads["0"]):
        assert torch.equal(ga, gb)
    for sa, sb in zip(stats["1"], stats["0"]):
        assert torch.equal(sa, sb)
